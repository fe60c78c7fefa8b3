// The policy-gradient criterion over B videos x S rollout rows (include/xgate_scst_video.h): RewardCriterion (xg_heads.hip:
// reward_fwd_kernel) with ONE score per row and the advantage formed here,
//
//   adv[b,s] = score[b,s] - baseline(b, s)      loss = sum -slp adv mask / sum mask      dslp = -scale adv mask / sum mask
//
// sv_reward_fwd_kernel    one 256-thread workgroup per video: thread s forms adv[b,s] (the other S - 1 scores added in index order),
//                         then the S L elements of the video are dealt to the threads round robin; a thread's terms add in index
//                         order, the wave's by wave_sum, the four waves' in wave order: the video's pair {sum, count} -> partial[b].
// sv_reward_sum_kernel    one wave adds the B pairs: lane l takes pairs l, l + 64, ... in index order, then wave_sum.
//                         Neither kernel takes a float atomic or reads its output: two identical calls give identical bits.
// sv_reward_bwd_kernel    one thread per element of dslp.
#include "xg_common.h"
#include "../../include/xgate_scst_video.h"

namespace {

constexpr int RT = 256, RW = RT / 64;

// RewardCriterion's mask (xg_heads.hip: reward_mask): column 0 always, column t when the row's word t - 1 is no end; none from n on
__device__ __forceinline__ float sv_mask(const int64_t* seq, int L, int64_t row, int t, int n) {
    if (t >= n) return 0.f;
    return (t == 0 || seq[row * L + t - 1] > 0) ? 1.f : 0.f;
}

__global__ void __launch_bounds__(RT) sv_reward_fwd_kernel(const float* __restrict__ slp, const int64_t* __restrict__ seq,
                                                           const float* __restrict__ score, const float* __restrict__ base,
                                                           int baseline, const int32_t* __restrict__ n_dev, int S, int L,
                                                           float* advantage, float* __restrict__ partial) {
    __shared__ float red[2 * RW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)b * S;
    const float* sc = score + row0;
    for (int s = tid; s < S; s += RT) {
        float a = sc[s];
        if (baseline == XGSV_BASE_MEAN_OTHERS) {
            float o = 0.f;
            for (int j = 0; j < S; ++j)
                if (j != s) o += sc[j];
            a -= o / (float)(S - 1);
        } else if (baseline == XGSV_BASE_GIVEN) {
            a -= base[b];
        }
        advantage[row0 + s] = a;
    }
    __syncthreads();                                  // the video's advantages are this workgroup's own stores
    int n = n_dev ? n_dev[0] : L;
    n = n < L ? n : L;
    float a = 0.f, k = 0.f;
    const int SL = S * L;
    for (int i = tid; i < SL; i += RT) {
        const int s = i / L, t = i - s * L;
        const float m = sv_mask(seq, L, row0 + s, t, n);
        if (m != 0.f) {
            a += -slp[(row0 + s) * L + t] * advantage[row0 + s];
            k += 1.f;
        }
    }
    a = wave_sum(a);
    k = wave_sum(k);
    if (lane == 0) { red[wave] = a; red[RW + wave] = k; }
    __syncthreads();
    if (tid == 0) {
        float sa = 0.f, sk = 0.f;
        for (int w = 0; w < RW; ++w) { sa += red[w]; sk += red[RW + w]; }
        partial[2 * b] = sa;
        partial[2 * b + 1] = sk;
    }
}

__global__ void __launch_bounds__(64) sv_reward_sum_kernel(const float* __restrict__ partial, int B, float* __restrict__ out) {
    const int lane = threadIdx.x;
    float a = 0.f, k = 0.f;
    for (int b = lane; b < B; b += 64) { a += partial[2 * b]; k += partial[2 * b + 1]; }
    a = wave_sum(a);
    k = wave_sum(k);
    if (lane == 0) { out[0] = a; out[1] = k; }
}

__global__ void __launch_bounds__(RT) sv_reward_bwd_kernel(const int64_t* __restrict__ seq, const float* __restrict__ advantage,
                                                           const int32_t* __restrict__ n_dev, int64_t ML, int L,
                                                           const float* __restrict__ sums, const float* __restrict__ scale_dev,
                                                           float* __restrict__ dslp) {
    const int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (i >= ML) return;
    const int64_t row = i / L;
    const int t = (int)(i - row * L);
    int n = n_dev ? n_dev[0] : L;
    n = n < L ? n : L;
    const float m = sv_mask(seq, L, row, t, n);
    dslp[i] = m != 0.f ? -(scale_dev ? scale_dev[0] : 1.f) * advantage[row] / sums[1] : 0.f;
}

inline bool sv_reward_dims_ok(int B, int S, int L) { return B >= 1 && S >= 1 && L >= 1 && (int64_t)B * S <= (1 << 20) && L <= (1 << 10); }

}  // namespace

extern "C" int xgsv_reward_fwd(void* stream, const float* seq_logp, const int64_t* seq, const float* score, const float* base,
                               int32_t baseline, const int32_t* n_dev, int32_t B, int32_t S, int32_t L, float* advantage,
                               float* partial, float* out) {
    if (!seq_logp || !seq || !score || !advantage || !partial || !out || !sv_reward_dims_ok(B, S, L)) return XG_EINVAL;
    if (baseline != XGSV_BASE_NONE && baseline != XGSV_BASE_MEAN_OTHERS && baseline != XGSV_BASE_GIVEN) return XG_EINVAL;
    if ((baseline == XGSV_BASE_MEAN_OTHERS && S < 2) || (baseline == XGSV_BASE_GIVEN && !base)) return XG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sv_reward_fwd_kernel, dim3(B), dim3(RT), 0, st, seq_logp, seq, score, base, baseline, n_dev, S, L, advantage,
                       partial);
    XG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sv_reward_sum_kernel, dim3(1), dim3(64), 0, st, partial, B, out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

extern "C" int xgsv_reward_bwd(void* stream, const int64_t* seq, const float* advantage, const int32_t* n_dev, int32_t B, int32_t S,
                               int32_t L, const float* sums, const float* scale_dev, float* dseq_logp) {
    if (!seq || !advantage || !sums || !dseq_logp || !sv_reward_dims_ok(B, S, L)) return XG_EINVAL;
    const int64_t ML = (int64_t)B * S * L;
    hipLaunchKernelGGL(sv_reward_bwd_kernel, dim3((unsigned)xg_cdiv64(ML, RT)), dim3(RT), 0, (hipStream_t)stream, seq, advantage, n_dev,
                       ML, L, sums, scale_dev, dseq_logp);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
