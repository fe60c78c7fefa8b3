// The attention backward for SEVERAL decoder rows of ONE video (include/xgate_train_video.h): teacher-forced training on Q captions
// per video keeps v2a(V) (B,K,A) and V (B,K,R) per VIDEO and p, alpha, af and their gradients per row, row b Q + q.  The
// expressions are xg_attn.hip's:
//
//   dalpha_k = daf . V_k      de_k = alpha_k (dalpha_k - sum_j alpha_j dalpha_j)      dp_a = w_a sum_k de_k (1 - tanh^2(p_a + q_ka))
//
// and, behind the reverse-time loop, what a video's rows send to the video's own tensors:
//
//   dq[b,k,a] = w_a sum_t sum_q de[t, b Q + q, k] (1 - tanh^2(P[t, b Q + q, a] + q[b,k,a]))      dw_a += sum de tanh(.)
//   dV[b,k,r] = sum_t sum_q alpha[t, b Q + q, k] daf[t, b Q + q, r]
//
// attn_bwd_group_kernel   one 512-thread workgroup serves up to G = 4 rows of one video and 512 attention columns.  The rows' daf
//                         vectors sit in LDS (G R floats); a wave takes whole V rows (lane = 16 B) ONCE and applies each to the G
//                         daf vectors; the softmax backward of row g is wave g's; then a thread owns ONE attention column and
//                         applies its K values of q, each once, to the G rows (p and the sums in registers, de in LDS).
//                         The 209 KB of a video (q and V at the real sizes) live nowhere: every element passes through a register
//                         once per group.  The kernel is bound by memory round trips, not by its 26 x 4 tanh per thread, so every
//                         load that depends on no other thread -- the column of q (32 frames), p, w_a, the wave's alpha row and its
//                         first 8 pieces of V -- is requested before the first barrier (docs/CAPTION_TRAIN_PER_VIDEO.md has the times).
//                         The column parts of a group repeat the dalpha dots (V is read cdiv(A, 512) times per group, from L2);
//                         part 0 writes de.  A row's sums run in one fixed order that knows neither the row's place in its group
//                         nor whether the group is full.
// attn_bwd_rows_kernel    every other shape: attn_bwd_kernel's loop, one workgroup per row, the video's operands at row / Q.
// attn_post_group_kernel  grid (column blocks of A + column blocks of R, B, frame parts): a thread owns one column of dq (or of dV)
//                         of one video for the workgroup's frames and walks the video's Q T (step, row) pairs in chunks of 16
//                         held in registers -- its column of P (of daf) -- against those frames; a chunk's de (alpha) is staged
//                         in LDS.  A video's tanh work is Q times a row's, so its frames are dealt to min(Q, K, 16) workgroups:
//                         as many threads as the per-row pass has.  ONE writer per element, the chunks added in (t, q) order: no
//                         float atomic on dq or dV.  dw_a is one atomic add per thread, as attn_post_dV_kernel has it.
// rows_sum_group_kernel   out[b, r] = sum_q in[b Q + q, r] in q order (the gradients of the initial state).
#include "xg_common.h"
#include "xg_kernels.h"

namespace {

constexpr int BG = XGK_ATTN_BWD_GROUP;    // rows of one video per workgroup
constexpr int BT = 512, BW = BT / 64;
constexpr int BRT = 512;

template <int G>
__global__ void __launch_bounds__(BT) attn_bwd_group_kernel(const float* __restrict__ daf, int lddaf, const float* __restrict__ p,
                                                            const float* __restrict__ vproj, const float* __restrict__ V,
                                                            const float* __restrict__ w, const float* __restrict__ alpha,
                                                            float* __restrict__ de, float* __restrict__ dp, int Q, int K, int R, int A,
                                                            int nparts) {
    static_assert(BW >= G, "the softmax backward of row g is wave g's");
    extern __shared__ float sm[];                     // daf (G, R) | dalpha, then de (G, K4)
    XG_CHAIN_PRIO();
    const int K4 = (K + 3) & ~3;
    float* dafs = sm;
    float* da = sm + (size_t)G * R;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = (Q + G - 1) / G;
    const int part = blockIdx.x % nparts, grp = blockIdx.x / nparts;
    const int b = grp / ng, g0 = (grp - b * ng) * G;
    const int cnt = Q - g0 < G ? Q - g0 : G;          // rows of this group (a video's last group may be partial)
    const size_t row0 = (size_t)b * Q + g0;
    const float* Vb = V + (size_t)b * K * R;
    const int a = part * BT + tid;                    // this thread's attention column
    const bool a_ok = a < A;
    // ---- everything that depends on no other thread is requested up front (one memory round trip): the thread's column of q for
    // the first QB frames, its p and w_a, the wave's row of alpha, the wave's first VB pieces of V, the group's daf rows
    constexpr int QB = 32, VB = 8;
    const float* qc = vproj + (size_t)b * K * A + (a_ok ? a : 0);
    float qv[QB];
#pragma unroll
    for (int k = 0; k < QB; ++k) qv[k] = (a_ok && k < K) ? qc[(size_t)k * A] : 0.f;
    float pa[G];
#pragma unroll
    for (int g = 0; g < G; ++g) pa[g] = (a_ok && g < cnt) ? p[(row0 + g) * A + a] : 0.f;
    const float wa = a_ok ? w[a] : 0.f;
    const float al0 = (wave < cnt && lane < K) ? alpha[(row0 + wave) * K + lane] : 0.f;
    // the wave's share of V: rows wave, wave + BW, ... as 16-byte pieces per lane, piece i = (row i / nch, 256-float chunk i % nch)
    const int nch = (R + 255) >> 8;
    const int nit = wave < K ? (K - wave + BW - 1) / BW * nch : 0;
    auto vload = [&](int i) {
        const int j = i / nch, c = i - j * nch, r = lane * 4 + 256 * c;
        return (i < nit && r < R) ? *reinterpret_cast<const float4*>(Vb + (size_t)(wave + j * BW) * R + r) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    float4 vb[VB];
#pragma unroll
    for (int u = 0; u < VB; ++u) vb[u] = vload(u);
    for (int i = tid * 4; i < cnt * R; i += BT * 4) { // (R % 4 == 0: a 16-byte piece never spans two rows)
        const int g = i / R, r = i - g * R;
        *reinterpret_cast<float4*>(dafs + i) = *reinterpret_cast<const float4*>(daf + (row0 + g) * lddaf + r);
    }
    __syncthreads();
    {   // dalpha[g][k] = daf_g . V_k: every piece of V once for the G rows
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        for (int i0 = 0; i0 < nit; i0 += VB) {
#pragma unroll
            for (int u = 0; u < VB; ++u) {
                const int i = i0 + u;
                if (i < nit) {                        // (wave-uniform, as is the end of a row below)
                    const int j = i / nch, c = i - j * nch, r = lane * 4 + 256 * c;
                    if (r < R) {
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            if (g < cnt) {
                                const float4 d4 = *reinterpret_cast<const float4*>(dafs + (size_t)g * R + r);
                                acc[g] += d4.x * vb[u].x + d4.y * vb[u].y + d4.z * vb[u].z + d4.w * vb[u].w;
                            }
                        }
                    }
                    if (c == nch - 1) {               // the row is complete: every lane takes part in the reduction
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            if (g < cnt) {
                                const float e = wave_sum(acc[g]);
                                if (lane == 0) da[g * K4 + wave + j * BW] = e;
                            }
                            acc[g] = 0.f;
                        }
                    }
                }
            }
            if (i0 + VB < nit) {
#pragma unroll
                for (int u = 0; u < VB; ++u) vb[u] = vload(i0 + VB + u);
            }
        }
    }
    __syncthreads();
    if (wave < cnt) {                                 // softmax backward of row g = wave, a lane per frame
        const int g = wave;
        const float* al = alpha + (row0 + g) * K;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += (k == lane ? al0 : al[k]) * da[g * K4 + k];
        const float dot = wave_sum(s);
        for (int k = lane; k < K; k += 64) {
            const float d = (k == lane ? al0 : al[k]) * (da[g * K4 + k] - dot);
            da[g * K4 + k] = d;
            if (part == 0) de[(row0 + g) * K + k] = d;
        }
    }
    __syncthreads();
    if (!a_ok) return;
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = 0.f;
    for (int k0 = 0; k0 < K; k0 += QB) {
        if (k0 > 0) {                                 // more than QB frames: the next block of the column
#pragma unroll
            for (int k = 0; k < QB; ++k) qv[k] = k0 + k < K ? qc[(size_t)(k0 + k) * A] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < QB; ++k) {
            if (k0 + k < K) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (g < cnt) {
                        const float th = xg_tanh(pa[g] + qv[k]);
                        s[g] += da[g * K4 + k0 + k] * (1.0f - th * th);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (g < cnt) dp[(row0 + g) * A + a] = s[g] * wa;
}

__global__ void __launch_bounds__(BRT) attn_bwd_rows_kernel(const float* __restrict__ daf, int lddaf, const float* __restrict__ p,
                                                            const float* __restrict__ vproj, const float* __restrict__ V,
                                                            const float* __restrict__ w, const float* __restrict__ alpha,
                                                            float* __restrict__ de, float* __restrict__ dp, int Q, int K, int R, int A) {
    extern __shared__ float sm[];          // dalpha[K] then de[K]
    const int row = blockIdx.x, b = row / Q;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = BRT / 64;
    const float* Vb = V + (size_t)b * K * R;
    const float* dafb = daf + (size_t)row * lddaf;
    for (int k = wave; k < K; k += nw) {
        float acc = 0.f;
        for (int r = lane; r < R; r += 64) acc += dafb[r] * Vb[(size_t)k * R + r];
        acc = wave_sum(acc);
        if (lane == 0) sm[k] = acc;
    }
    __syncthreads();
    float dot = 0.f;
    for (int k = 0; k < K; ++k) dot += alpha[(size_t)row * K + k] * sm[k];
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += BRT) {
        const float d = alpha[(size_t)row * K + k] * (sm[k] - dot);
        sm[k] = d;
        de[(size_t)row * K + k] = d;
    }
    __syncthreads();
    const float* pb = p + (size_t)row * A;
    const float* qb = vproj + (size_t)b * K * A;
    for (int a = threadIdx.x; a < A; a += BRT) {
        const float pa = pb[a];
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            const float th = xg_tanh(pa + qb[(size_t)k * A + a]);
            s += sm[k] * (1.0f - th * th);
        }
        dp[(size_t)row * A + a] = s * w[a];
    }
}

constexpr int PT = 256, PCH = 16;
constexpr int PKMAX = 512;                // frames per workgroup at most: a chunk's PCH x PKMAX coefficients are 32 KB of LDS

// grid (column blocks of A + column blocks of R, B, frame parts): the workgroup's frames are [z kper, min(K, (z + 1) kper))
__global__ void __launch_bounds__(PT) attn_post_group_kernel(const float* __restrict__ P, const float* __restrict__ vproj,
                                                             const float* __restrict__ w, const float* __restrict__ DE,
                                                             float* __restrict__ dvproj, float* __restrict__ dw,
                                                             const float* __restrict__ ALPHA, const float* __restrict__ DAF, int lddaf,
                                                             int64_t tstride, float* __restrict__ dV, int T, int B, int Q, int K, int A,
                                                             int R, int nxa, int kper) {
    extern __shared__ float sc[];                     // (PCH, kn): de (alpha) of one chunk's (step, row) pairs, zeros past the last pair
    const int b = blockIdx.y, tid = threadIdx.x;
    const bool is_a = (int)blockIdx.x < nxa;          // the attention columns (dq, dw) or the context columns (dV)
    const int TQ = T * Q;
    const int k0 = blockIdx.z * kper, kn = min(K - k0, kper);
    const size_t M = (size_t)B * Q, vrow0 = (size_t)b * Q;
    const float* src = is_a ? DE : ALPHA;
    const int C = is_a ? A : R;
    const int c = ((int)blockIdx.x - (is_a ? 0 : nxa)) * PT + tid;
    const bool live = c < C;                          // (threads past the last column still stage and meet the barriers)
    const int cc = live ? c : 0;
    const float wa = is_a ? w[cc] : 0.f;
    float* out = (is_a ? dvproj : dV) + ((size_t)b * K + k0) * C + cc;
    const float* qcol = vproj + ((size_t)b * K + k0) * A + (is_a ? cc : 0);
    float dwa = 0.f;
    for (int j0 = 0; j0 < TQ; j0 += PCH) {
        float x[PCH];                                 // this thread's column of P (of daf) for the chunk's (step, row) pairs
#pragma unroll
        for (int jj = 0; jj < PCH; ++jj) {
            const int j = min(j0 + jj, TQ - 1), t = j / Q, q = j - t * Q;
            const float v = is_a ? P[((size_t)t * M + vrow0 + q) * A + cc] : DAF[(size_t)t * tstride + (vrow0 + q) * lddaf + cc];
            x[jj] = j0 + jj < TQ ? v : 0.f;
        }
        __syncthreads();                              // the chunk before this one has been read
        for (int i = tid; i < PCH * kn; i += PT) {
            const int jj = i / kn, k = i - jj * kn, j = j0 + jj, t = j / Q, q = j - t * Q;
            sc[i] = j < TQ ? src[((size_t)t * M + vrow0 + q) * K + k0 + k] : 0.f;
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < kn; ++k) {
                float acc = 0.f;
                const float qv = is_a ? qcol[(size_t)k * A] : 0.f;
#pragma unroll
                for (int jj = 0; jj < PCH; ++jj) {
                    const float d = sc[jj * kn + k];
                    if (is_a) {
                        const float th = xg_tanh(x[jj] + qv);
                        acc += d * (1.0f - th * th);
                        dwa += d * th;
                    } else {
                        acc += d * x[jj];
                    }
                }
                if (is_a) acc *= wa;
                float* o = out + (size_t)k * C;
                *o = j0 == 0 ? acc : *o + acc;        // (this thread is the element's only writer: the chunks add in (t, q) order)
            }
        }
    }
    if (live && is_a && dw) atomicAdd(dw + c, dwa);
}

__global__ void __launch_bounds__(256) rows_sum_group_kernel(const float* __restrict__ in, float* __restrict__ out, int Q, int R,
                                                             int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / R, r = i - b * R;
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += in[(b * Q + q) * R + r];
    out[i] = s;
}

inline bool group_shape_ok(int B, int Q, int K) { return B >= 1 && Q >= 1 && K >= 1 && K <= 8192 && (int64_t)B * Q <= (1 << 20); }

}  // namespace

int xgk_attn_bwd_group_form(const float* daf, int lddaf, const float* p, const float* vproj, const float* V, const float* w,
                            const float* dp, int K, int R, int A) {
    const bool al16 = ((uintptr_t)daf % 16 == 0) && ((uintptr_t)p % 16 == 0) && ((uintptr_t)vproj % 16 == 0) && ((uintptr_t)V % 16 == 0) &&
                      ((uintptr_t)w % 16 == 0) && ((uintptr_t)dp % 16 == 0);
    const size_t lds = ((size_t)BG * R + (size_t)BG * ((K + 3) & ~3)) * sizeof(float);
    return (al16 && A % 4 == 0 && R % 4 == 0 && lddaf % 4 == 0 && lds <= 60000) ? 1 : 0;
}

int xgk_attn_bwd_group(hipStream_t st, const float* daf, int lddaf, const float* p, const float* vproj, const float* V, const float* w,
                       const float* alpha, float* de, float* dp, int B, int Q, int K, int R, int A) {
    if (!group_shape_ok(B, Q, K) || R < 1 || A < 1) return XG_EINVAL;
    if (xgk_attn_bwd_group_form(daf, lddaf, p, vproj, V, w, dp, K, R, A)) {
        const int nparts = xg_cdiv(A, BT);
        const int64_t grid = (int64_t)B * xg_cdiv(Q, BG) * nparts;
        if (grid > 0x7FFFFFFF) return XG_EINVAL;
        const size_t lds = ((size_t)BG * R + (size_t)BG * ((K + 3) & ~3)) * sizeof(float);
        hipLaunchKernelGGL((attn_bwd_group_kernel<BG>), dim3((unsigned)grid), dim3(BT), lds, st, daf, lddaf, p, vproj, V, w, alpha, de, dp,
                           Q, K, R, A, nparts);
    } else {
        hipLaunchKernelGGL(attn_bwd_rows_kernel, dim3(B * Q), dim3(BRT), K * sizeof(float), st, daf, lddaf, p, vproj, V, w, alpha, de, dp,
                           Q, K, R, A);
    }
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_attn_post_dV_group(hipStream_t st, const float* P, const float* vproj, const float* w, const float* DE, float* dvproj, float* dw,
                           const float* ALPHA, const float* DAF, int lddaf, int64_t daf_tstride, float* dV, int T, int B, int Q, int K,
                           int A, int R) {
    if (!group_shape_ok(B, Q, K) || T < 1 || R < 1 || A < 1 || B > 65535 || (int64_t)T * Q > (1 << 24)) return XG_EINVAL;
    const int nxa = xg_cdiv(A, PT), nxr = xg_cdiv(R, PT);
    // the frames of a video go to as many workgroups as it has rows (the tanh work of a video is Q times a row's), 16 at most, and
    // to as many as keep a workgroup's frames within PKMAX
    int nkz = Q < 16 ? Q : 16;
    if (nkz > K) nkz = K;
    if (nkz < xg_cdiv(K, PKMAX)) nkz = xg_cdiv(K, PKMAX);
    const int kper = xg_cdiv(K, nkz);
    nkz = xg_cdiv(K, kper);                           // (no workgroup without a frame)
    const dim3 grid(nxa + nxr, B, nkz);
    const size_t lds = (size_t)PCH * kper * sizeof(float);
    hipLaunchKernelGGL(attn_post_group_kernel, grid, dim3(PT), lds, st, P, vproj, w, DE, dvproj, dw, ALPHA, DAF, lddaf, daf_tstride, dV,
                       T, B, Q, K, A, R, nxa, kper);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_rows_sum_group(hipStream_t st, const float* in, float* out, int B, int Q, int R) {
    if (B < 1 || Q < 1 || R < 1) return XG_EINVAL;
    const int64_t n = (int64_t)B * R;
    hipLaunchKernelGGL(rows_sum_group_kernel, dim3((unsigned)xg_cdiv64(n, 256)), dim3(256), 0, st, in, out, Q, R, n);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
