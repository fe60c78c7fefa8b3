// Kernels of the captioner's beam search (include/xgate_beam.h; the host loop is xgcb_beam_search in xg_model.hip).
//
// Per step, after the decoder step (core_step) and the vocabulary product over the M = B W rows:
//   cap_beam_topw_kernel   one workgroup per row: log-sum-exp of the row's V logits and its W best (lp, word) pairs.  The (M,V)
//                          log-softmax is never written.  The row is read from memory ONCE and staged in LDS (80 KB at V = 20000);
//                          a row beyond 150 KiB is read three times instead.  Ranking is on lp = logit - lse itself, so two
//                          logits that round to one lp are ordered by word index like the host search's torch.topk over lp.
//   cap_beam_topw_thr_kernel  the same outputs, the insertion replaced by a threshold from the threads' maxima and a short candidate
//                          list (the search over S templates per video, include/xgate_beam_control.h, has S times the rows).
//   cap_beam_topw_allow_kernel  the threshold form over a row's ALLOWED words (include/xgate_beam_allow.h): the log-sum-exp runs over
//                          them alone and every other word is lowered by 1000 like the suppressed one.
//   cap_beam_topw_rules_kernel  either threshold form with 1000 more off the words a row's history bans (include/xgate_beam_rules.h):
//                          the ban is applied to the <= L + 1 banned elements alone.
//   cap_beam_merge_kernel  one workgroup per video: fills the candidate tables from topv / topi, runs steps 3-5 of the rule
//                          (beam_merge, xg_beam_core.h), and every thread gathers h1, c1, h2, c2 of slot v from its parent out of
//                          the step's OUTPUT buffer into its INPUT buffer.
// After the loop cap_beam_backtrace_kernel follows each done entry's parents back (beam_backtrace_row).  cap_beam_repeat_kernel
// row-repeats what was computed once per video (xgk_compact copies contiguous blocks: rows b W + slot of video b are not one).
#include "xg_common.h"
#include "xg_kernels.h"
#include "../../include/xgate_beam_rules.h"

namespace {

constexpr int CB_TPB = 256;
// the top-W kernel's workgroup: a row of V = 20000 is 20 elements a thread (38 -> 31 us over 320 rows against 256 threads;
// docs/CAPTION_BEAM.md has what else was measured)
constexpr int TW_TPB = 1024, TW_WAVES = TW_TPB / 64;
constexpr int CB_MAX = XG_BEAM_MAX;
constexpr int CB_EMPTY = 0x7fffffff;                      // word index of a list entry that holds nothing
constexpr int CB_STAGE_BYTES = 150 * 1024;                // the most dynamic LDS a row may take (as xgk_rollout_step)
constexpr int TW_CAND = 32;                               // the threshold form's candidate list (cap_beam_topw_thr_kernel): 4 W at the widest
static_assert(TW_WAVES * CB_MAX <= TW_TPB, "one thread per entry of the last ranking");
static_assert(TW_CAND <= TW_TPB && TW_CAND >= CB_MAX, "one thread per candidate; room for W of them");

// One row of logits as the top-W kernels see it: staged in LDS after its one trip from memory, or (a row beyond CB_STAGE_BYTES)
// read from memory by every pass.
template <bool STAGE>
struct TopwRow {
    const float* g; const float4* g4; float* row;
    int V, tid, head, nvec, tail0;
    __device__ __forceinline__ TopwRow(const float* logits, int64_t ld, int V_, float4* lds4) : V(V_), tid(threadIdx.x) {
        g = logits + (size_t)blockIdx.x * ld;
        // rows of a V that is no multiple of 4 start off the 16-byte grid: `head` scalars, `nvec` float4, the rest scalars
        const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
        head = min(V, (4 - mis) & 3);
        nvec = (V - head) >> 2;
        tail0 = head + 4 * nvec;
        g4 = reinterpret_cast<const float4*>(g + head);
        row = reinterpret_cast<float*>(lds4) + mis;               // (row + head is on the 16-byte grid like g + head)
    }
    template <typename F>
    __device__ __forceinline__ void each_global(F&& f) const {
        if (tid < head) f(g[tid], tid);
        for (int j = tid; j < nvec; j += TW_TPB) {
            const float4 x = g4[j];
            const int i = head + 4 * j;
            f(x.x, i); f(x.y, i + 1); f(x.z, i + 2); f(x.w, i + 3);
        }
        if (tail0 + tid < V) f(g[tail0 + tid], tail0 + tid);
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
        if constexpr (STAGE) { for (int i = tid; i < V; i += TW_TPB) f(row[i], i); }
        else each_global(f);
    }
    // the row's maximum (and, staged, its one trip from memory), then its log-sum-exp; red: TW_WAVES floats of LDS
    __device__ __forceinline__ float stage_lse(float* red) const {
        const int lane = tid & 63, wave = tid >> 6;
        float mx = -INFINITY;
        if constexpr (STAGE) {
            if (tid < head) { const float x = g[tid]; row[tid] = x; mx = fmaxf(mx, x); }
            for (int j = tid; j < nvec; j += TW_TPB) {
                const float4 x = g4[j];
                *reinterpret_cast<float4*>(row + head + 4 * j) = x;
                mx = fmaxf(fmaxf(mx, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
            }
            if (tail0 + tid < V) { const float x = g[tail0 + tid]; row[tail0 + tid] = x; mx = fmaxf(mx, x); }
        } else {
            each_global([&](float x, int) { mx = fmaxf(mx, x); });
        }
        mx = wave_max(mx);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
#pragma unroll
        for (int k = 1; k < TW_WAVES; ++k) mx = fmaxf(mx, red[k]);
        __syncthreads();
        // log-sum-exp: thread, wave (DPP), then the waves in one fixed order
        float s = 0.f;
        each([&](float x, int) { s += __expf(x - mx); });
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < TW_WAVES; ++k) tot += red[k];
        return mx + logf(tot);
    }
};

// The selection by insertion, called by ALL threads of the workgroup: each thread's W best of its elements in registers, a wave's W
// best by W rounds of a shuffle arg-max, the last waves * W entries by counting.  cv / ci: TW_WAVES * W entries of LDS.
template <int W, bool STAGE>
__device__ __forceinline__ void topw_by_insertion(const TopwRow<STAGE>& r, float lse, int suppress, float* cv, int* ci,
                                                  float* __restrict__ topv, int32_t* __restrict__ topi) {
    const int tid = r.tid, lane = tid & 63, wave = tid >> 6, V = r.V;
    // ---- each thread's W best in registers (a descending list; unrolled insertion, no indexing by a variable)
    float bv[W];
    int bi[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { bv[k] = -INFINITY; bi[k] = CB_EMPTY; }
    r.each([&](float x, int i) {
        float v = x - lse;
        if (i == suppress) v -= 1000.0f;
        int ix = i;
        if (beam_before(v, ix, bv[W - 1], bi[W - 1])) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (beam_before(v, ix, bv[k], bi[k])) {         // from here on v is what the list pushes down
                    const float tv = bv[k]; const int ti = bi[k];
                    bv[k] = v; bi[k] = ix; v = tv; ix = ti;
                }
            }
        }
    });
    // ---- the wave's W best: W rounds of (best head of any lane, that lane pops)
#pragma unroll
    for (int rd = 0; rd < W; ++rd) {
        float v = bv[0];
        int ix = bi[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(ix, off);
            if (beam_before(ov, oi, v, ix)) { v = ov; ix = oi; }
        }
        if (lane == 0) { cv[wave * W + rd] = v; ci[wave * W + rd] = ix; }
        if (bi[0] == ix) {
#pragma unroll
            for (int k = 0; k + 1 < W; ++k) { bv[k] = bv[k + 1]; bi[k] = bi[k + 1]; }
            bv[W - 1] = -INFINITY; bi[W - 1] = CB_EMPTY;
        }
    }
    __syncthreads();
    // ---- the last waves * W entries by counting; the position breaks ties among empty entries, so every rank is taken once and
    // every output is written (an empty entry, which only a row with NaNs leaves, becomes word 0 at -inf)
    if (tid < TW_WAVES * W) {
        const float v = cv[tid];
        const int ix = ci[tid];
        int rank = 0;
        for (int j = 0; j < TW_WAVES * W; ++j) {
            const float ov = cv[j];
            const int oi = ci[j];
            rank += (beam_before(ov, oi, v, ix) || (ov == v && oi == ix && j < tid)) ? 1 : 0;
        }
        if (rank < W) {
            topv[(size_t)blockIdx.x * W + rank] = v;
            topi[(size_t)blockIdx.x * W + rank] = (ix >= 0 && ix < V) ? ix : 0;
        }
    }
}

template <int W, bool STAGE>
__global__ void __launch_bounds__(TW_TPB) cap_beam_topw_kernel(const float* __restrict__ logits, int64_t ld, int V, int suppress,
                                                               float* __restrict__ topv, int32_t* __restrict__ topi) {
    extern __shared__ float4 cb_lds4[];
    __shared__ float red[TW_WAVES], cv[TW_WAVES * W];
    __shared__ int ci[TW_WAVES * W];
    const TopwRow<STAGE> r(logits, ld, V, cb_lds4);
    const float lse = r.stage_lse(red);
    topw_by_insertion<W, STAGE>(r, lse, suppress, cv, ci, topv, topi);
}

// The same contract and outputs with the selection behind a THRESHOLD (include/xgate_beam_control.h; only xgbc_beam_search
// launches it).  tau = the W-th largest of the threads' maxima of v = lp (less 1000 at `suppress`): every thread's maximum is
// another element of the row and min(V, TW_TPB) >= W threads hold one, so at least W elements have v >= tau and every member of the
// top W has.  A second pass collects the elements with v >= tau in LDS (the list's order never reaches the output: an LDS atomic
// counts them) and the list is ranked by counting on beam_before, ties at tau included.  A list outside [W, TW_CAND] -- many
// exact ties at tau; none at all in a row with NaNs, where no comparison holds -- sends the WHOLE workgroup to the insertion path.
template <int W, bool STAGE>
__global__ void __launch_bounds__(TW_TPB) cap_beam_topw_thr_kernel(const float* __restrict__ logits, int64_t ld, int V, int suppress,
                                                                   float* __restrict__ topv, int32_t* __restrict__ topi) {
    extern __shared__ float4 cb_lds4[];
    __shared__ float red[TW_WAVES], cv[TW_WAVES * W], lv[TW_CAND], tau_s;
    __shared__ int ci[TW_WAVES * W], li[TW_CAND], cnt_s;
    const TopwRow<STAGE> r(logits, ld, V, cb_lds4);
    const int tid = r.tid, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) cnt_s = 0;                                      // (two barriers in stage_lse come before its first use)
    const float lse = r.stage_lse(red);
    // ---- each thread's maximum, a wave's W largest of those (W rounds: the wave's maximum, its first holder gives it up)
    float tm = -INFINITY;
    r.each([&](float x, int i) {
        float v = x - lse;
        if (i == suppress) v -= 1000.0f;
        tm = fmaxf(tm, v);
    });
#pragma unroll
    for (int rd = 0; rd < W; ++rd) {
        const float m = wave_max(tm);
        const unsigned long long holders = __ballot(tm == m);
        if (lane == 0) cv[wave * W + rd] = m;
        if (holders != 0 && lane == __ffsll(holders) - 1) tm = -INFINITY;
    }
    __syncthreads();
    // ---- tau: the W-th largest of the waves * W values, with multiplicity (the position breaks ties: one entry has rank W - 1)
    if (tid < TW_WAVES * W) {
        const float v = cv[tid];
        int rank = 0;
        for (int j = 0; j < TW_WAVES * W; ++j) {
            const float ov = cv[j];
            rank += (ov > v || (ov == v && j < tid)) ? 1 : 0;
        }
        if (rank == W - 1) tau_s = v;
    }
    __syncthreads();
    const float tau = tau_s;
    // ---- the candidates
    r.each([&](float x, int i) {
        float v = x - lse;
        if (i == suppress) v -= 1000.0f;
        if (v >= tau) {
            const int at = atomicAdd(&cnt_s, 1);
            if (at < TW_CAND) { lv[at] = v; li[at] = i; }
        }
    });
    __syncthreads();
    const int n = cnt_s;
    if (n < W || n > TW_CAND) {                                   // uniform over the workgroup
        topw_by_insertion<W, STAGE>(r, lse, suppress, cv, ci, topv, topi);
        return;
    }
    // ---- n >= W distinct words under a total order: every rank below W is taken exactly once, so every output is written
    if (tid < n) {
        const float v = lv[tid];
        const int ix = li[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += beam_before(lv[j], li[j], v, ix) ? 1 : 0;
        if (rank < W) {
            topv[(size_t)blockIdx.x * W + rank] = v;
            topi[(size_t)blockIdx.x * W + rank] = ix;             // (an index of `each`: inside [0, V))
        }
    }
}

// ---- the selection under a per-row set of ALLOWED words (include/xgate_beam_allow.h; only xgba_beam_search launches it)
// Which of the row's words are allowed: word i iff bit (word_cat[i] & 31) of the row's mask.  Staged, a thread's elements are
// i = tid + k TW_TPB in every pass over LDS, so the predicate is ONE bit per element in a 64-bit register, built by one coalesced
// pass of byte loads over word_cat; unstaged, every pass reads the byte again beside the row (docs/CAPTION_ALLOW.md).
static_assert(CB_STAGE_BYTES / 4 <= 64 * TW_TPB, "a staged row's elements per thread fit the 64-bit predicate");
template <bool STAGE>
struct TopwAllowed {
    const uint8_t* cat; uint32_t mask; unsigned long long bits;
    __device__ __forceinline__ bool operator()(int i) const {
        if constexpr (STAGE) return (bits >> (i >> 10)) & 1ull;
        else return (mask >> (cat[i] & 31)) & 1u;
    }
};
static_assert(TW_TPB == 1 << 10, "TopwAllowed: element i of a staged row is bit i >> 10 of its thread");

// topw_by_insertion with the value of an element left to the caller (val(x, i); the source of cap_beam_topw_kernel's selection
// stays as it is: docs/CAPTION_BEAM_CONTROL.md on what re-factoring it did to its machine code)
template <int W, bool STAGE, typename Val>
__device__ __forceinline__ void topw_by_insertion_of(const TopwRow<STAGE>& r, Val&& val, float* cv, int* ci, float* __restrict__ topv,
                                                     int32_t* __restrict__ topi) {
    const int tid = r.tid, lane = tid & 63, wave = tid >> 6, V = r.V;
    float bv[W];
    int bi[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { bv[k] = -INFINITY; bi[k] = CB_EMPTY; }
    r.each([&](float x, int i) {
        float v = val(x, i);
        int ix = i;
        if (beam_before(v, ix, bv[W - 1], bi[W - 1])) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (beam_before(v, ix, bv[k], bi[k])) {
                    const float tv = bv[k]; const int ti = bi[k];
                    bv[k] = v; bi[k] = ix; v = tv; ix = ti;
                }
            }
        }
    });
#pragma unroll
    for (int rd = 0; rd < W; ++rd) {
        float v = bv[0];
        int ix = bi[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(ix, off);
            if (beam_before(ov, oi, v, ix)) { v = ov; ix = oi; }
        }
        if (lane == 0) { cv[wave * W + rd] = v; ci[wave * W + rd] = ix; }
        if (bi[0] == ix) {
#pragma unroll
            for (int k = 0; k + 1 < W; ++k) { bv[k] = bv[k + 1]; bi[k] = bi[k + 1]; }
            bv[W - 1] = -INFINITY; bi[W - 1] = CB_EMPTY;
        }
    }
    __syncthreads();
    if (tid < TW_WAVES * W) {
        const float v = cv[tid];
        const int ix = ci[tid];
        int rank = 0;
        for (int j = 0; j < TW_WAVES * W; ++j) {
            const float ov = cv[j];
            const int oi = ci[j];
            rank += (beam_before(ov, oi, v, ix) || (ov == v && oi == ix && j < tid)) ? 1 : 0;
        }
        if (rank < W) {
            topv[(size_t)blockIdx.x * W + rank] = v;
            topi[(size_t)blockIdx.x * W + rank] = (ix >= 0 && ix < V) ? ix : 0;
        }
    }
}

// The contract and outputs of cap_beam_topw_thr_kernel with lp = logit - lse_a, lse_a the log-sum-exp over the row's ALLOWED words,
// less 1000 at every word that is not allowed and less 1000 at `suppress`.  Row m belongs to group m / W and its mask is
// allow[(m / W) * astride] (the step's column of the (G,L) table).  A mask that admits no word of the vocabulary counts as all ones.
template <int W, bool STAGE>
__global__ void __launch_bounds__(TW_TPB) cap_beam_topw_allow_kernel(const float* __restrict__ logits, int64_t ld, int V, int suppress,
                                                                     const uint8_t* __restrict__ word_cat,
                                                                     const uint32_t* __restrict__ allow, int64_t astride,
                                                                     float* __restrict__ topv, int32_t* __restrict__ topi) {
    extern __shared__ float4 cb_lds4[];
    __shared__ float red[TW_WAVES], cv[TW_WAVES * W], lv[TW_CAND], tau_s;
    __shared__ int ci[TW_WAVES * W], li[TW_CAND], cnt_s, any_w[TW_WAVES];
    const TopwRow<STAGE> r(logits, ld, V, cb_lds4);
    const int tid = r.tid, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) cnt_s = 0;                                      // (barriers below come before its first use)
    TopwAllowed<STAGE> ok{word_cat, allow[(size_t)(blockIdx.x / W) * astride], 0ull};
    // ---- the row's one trip from memory (staged) and the predicate; does the mask admit any word at all?
    bool any = false;
    if constexpr (STAGE) {
        for (int i = tid, k = 0; i < V; i += TW_TPB, ++k)
            ok.bits |= (unsigned long long)((ok.mask >> (word_cat[i] & 31)) & 1u) << k;
        any = ok.bits != 0;
        if (tid < r.head) r.row[tid] = r.g[tid];
        for (int j = tid; j < r.nvec; j += TW_TPB) *reinterpret_cast<float4*>(r.row + r.head + 4 * j) = r.g4[j];
        if (r.tail0 + tid < V) r.row[r.tail0 + tid] = r.g[r.tail0 + tid];
    } else {
        for (int i = tid; i < V; i += TW_TPB) any = any || ok(i);
    }
    const unsigned long long some = __ballot(any);
    if (lane == 0) any_w[wave] = some != 0 ? 1 : 0;
    __syncthreads();                                              // (the staged row is complete behind it too)
    int found = 0;
#pragma unroll
    for (int k = 0; k < TW_WAVES; ++k) found |= any_w[k];
    if (!found) { ok.mask = 0xFFFFFFFFu; ok.bits = ~0ull; }       // uniform over the workgroup: never an empty softmax
    // ---- maximum and log-sum-exp over the allowed words: thread, wave (DPP), then the waves in one fixed order
    float mx = -INFINITY;
    r.each([&](float x, int i) { if (ok(i)) mx = fmaxf(mx, x); });
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int k = 1; k < TW_WAVES; ++k) mx = fmaxf(mx, red[k]);
    __syncthreads();
    float s = 0.f;
    r.each([&](float x, int i) { if (ok(i)) s += __expf(x - mx); });
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < TW_WAVES; ++k) tot += red[k];
    const float lse = mx + logf(tot);
    auto val = [&](float x, int i) {
        float v = x - lse;
        if (!ok(i)) v -= 1000.0f;
        if (i == suppress) v -= 1000.0f;
        return v;
    };
    // ---- the threshold selection of cap_beam_topw_thr_kernel over val
    float tm = -INFINITY;
    r.each([&](float x, int i) { tm = fmaxf(tm, val(x, i)); });
#pragma unroll
    for (int rd = 0; rd < W; ++rd) {
        const float m = wave_max(tm);
        const unsigned long long holders = __ballot(tm == m);
        if (lane == 0) cv[wave * W + rd] = m;
        if (holders != 0 && lane == __ffsll(holders) - 1) tm = -INFINITY;
    }
    __syncthreads();
    if (tid < TW_WAVES * W) {
        const float v = cv[tid];
        int rank = 0;
        for (int j = 0; j < TW_WAVES * W; ++j) {
            const float ov = cv[j];
            rank += (ov > v || (ov == v && j < tid)) ? 1 : 0;
        }
        if (rank == W - 1) tau_s = v;
    }
    __syncthreads();
    const float tau = tau_s;
    r.each([&](float x, int i) {
        const float v = val(x, i);
        if (v >= tau) {
            const int at = atomicAdd(&cnt_s, 1);
            if (at < TW_CAND) { lv[at] = v; li[at] = i; }
        }
    });
    __syncthreads();
    const int n = cnt_s;
    if (n < W || n > TW_CAND) {                                   // uniform over the workgroup
        topw_by_insertion_of<W, STAGE>(r, val, cv, ci, topv, topi);
        return;
    }
    if (tid < n) {
        const float v = lv[tid];
        const int ix = li[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += beam_before(lv[j], li[j], v, ix) ? 1 : 0;
        if (rank < W) {
            topv[(size_t)blockIdx.x * W + rank] = v;
            topi[(size_t)blockIdx.x * W + rank] = ix;             // (an index of `each`: inside [0, V))
        }
    }
}

template <int W>
int launch_topw_allow(hipStream_t st, const float* logits, int64_t ld, int M, int V, int suppress, const uint8_t* word_cat,
                      const uint32_t* allow, int64_t astride, float* topv, int32_t* topi) {
    const size_t lds = ((size_t)V + 8) * sizeof(float);
    if (lds <= (size_t)CB_STAGE_BYTES) {
        if (lds > 64 * 1024) {
            static std::atomic<unsigned> optin{0};
            XG_TRY(xg_lds_optin(optin, reinterpret_cast<const void*>(cap_beam_topw_allow_kernel<W, true>), CB_STAGE_BYTES));
        }
        hipLaunchKernelGGL((cap_beam_topw_allow_kernel<W, true>), dim3(M), dim3(TW_TPB), lds, st, logits, ld, V, suppress, word_cat,
                           allow, astride, topv, topi);
    } else {
        hipLaunchKernelGGL((cap_beam_topw_allow_kernel<W, false>), dim3(M), dim3(TW_TPB), 0, st, logits, ld, V, suppress, word_cat,
                           allow, astride, topv, topi);
    }
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// ---- the selection under RULES (include/xgate_beam_rules.h; only xgbr_beam_search launches it): cap_beam_topw_allow_kernel (ALLOW) or
// cap_beam_topw_thr_kernel (no template constraint) with 1000 more off every word of the row's banned set.  The log-sum-exp is the
// unbanned one, summed in the order of those kernels, so an empty set gives their bits.
// Prologue: the row's t <= L history tokens go to LDS; thread i < t - n + 1 compares the n - 1 words from start i with the last n - 1
// and names h[i+n-1] on a match, one more entry is word 0 (t < min_length, or wave 0 found h[t-1] in bad_end); an entry whose word an
// earlier entry names is dropped, so a word is lowered ONCE.  The <= L + 1 entries (holes: -1) and their exact values
// ((x - lse) - ..) - 1000 stand behind the row in dynamic LDS.
// Staged, entry j's thread then overwrites element w of the row with a quiet NaN whose payload is j: the passes over the row test
// x != x -- one compare per element, no list -- and only the <= L + 1 marked elements read their value from the list.  Unstaged (a row
// beyond CB_STAGE_BYTES is never written), an index inside [lowest, highest banned word] walks the list.
constexpr int RB_LMAX = XGBR_MAX_LENGTH;
constexpr int RB_EXTRA_BYTES = 2 * (RB_LMAX + 1) * 4;
static_assert(RB_LMAX + 1 <= TW_TPB, "one thread per entry of the ban list");
static_assert(CB_STAGE_BYTES + RB_EXTRA_BYTES + 2048 <= 160 * 1024, "row, history and ban list, and the static tables, fit the CU's LDS");
static_assert(RB_LMAX + 1 < (1 << 22), "an entry's index fits a quiet NaN's payload");

template <int W, bool STAGE, bool ALLOW>
__global__ void __launch_bounds__(TW_TPB) cap_beam_topw_rules_kernel(const float* __restrict__ logits, int64_t ld, int V, int suppress,
                                                                     const uint8_t* __restrict__ word_cat,
                                                                     const uint32_t* __restrict__ allow, int64_t astride, CapBeamBan ban,
                                                                     int row_floats, float* __restrict__ topv, int32_t* __restrict__ topi) {
    extern __shared__ float4 cb_lds4[];
    __shared__ float red[TW_WAVES], cv[TW_WAVES * W], lv[TW_CAND], tau_s;
    __shared__ int ci[TW_WAVES * W], li[TW_CAND], cnt_s, any_w[TW_WAVES], ban0_s, lo_s, hi_s;
    const TopwRow<STAGE> r(logits, ld, V, cb_lds4);
    const int tid = r.tid, lane = tid & 63, wave = tid >> 6;
    int* bw = reinterpret_cast<int*>(cb_lds4) + row_floats;       // (L + 1) the banned words, -1: a hole
    int* hs = bw + (ban.L + 1);                                   // (L) the history; dead once bw stands, then
    float* bx = reinterpret_cast<float*>(hs);                     // (L + 1) the entries' values
    const int t = ban.t, n = ban.ngram;
    auto word = [&](int w) { return w < 0 ? 0 : (w >= V ? V - 1 : w); };
    if (tid == 0) { cnt_s = 0; lo_s = 0x7fffffff; hi_s = -1; }    // (barriers below come before their first use)
    // ---- the history, and the two conditions on word 0
    const int32_t* h = ban.hist + (size_t)blockIdx.x * ban.L;
    for (int i = tid; i < t; i += TW_TPB) hs[i] = word(h[i]);
    if (wave == 0) {
        bool hit = false;
        if (t >= 1 && lane < ban.n_bad_end) hit = word(ban.bad_end[lane]) == word(h[t - 1]);
        const unsigned long long hits = __ballot(hit);
        if (lane == 0) ban0_s = (t < ban.min_length || hits != 0) ? 1 : 0;
    }
    __syncthreads();
    // ---- the entries: one per start of an earlier n-gram, then word 0's
    const int ng = (n >= 1 && t >= n) ? t - n + 1 : 0, nslots = ng + 1;
    if (tid < ng) {
        bool same = true;
        for (int k = 0; k + 1 < n; ++k) same = same && hs[tid + k] == hs[t - n + 1 + k];
        bw[tid] = same ? hs[tid + n - 1] : -1;
    }
    if (tid == ng) bw[ng] = ban0_s ? 0 : -1;
    __syncthreads();
    int mine = -1;                                                // entry tid's word, if no earlier entry names it
    if (tid < nslots) {
        mine = bw[tid];
        for (int j = 0; j < tid && mine >= 0; ++j) mine = bw[j] == mine ? -1 : mine;
    }
    __syncthreads();
    if (tid < nslots) {
        bw[tid] = mine;
        if (mine >= 0) { atomicMin(&lo_s, mine); atomicMax(&hi_s, mine); }
    }
    // ---- the row's one trip from memory (staged) and its log-sum-exp, as the kernel without rules forms it
    TopwAllowed<STAGE> ok{word_cat, 0u, 0ull};
    float lse;
    if constexpr (ALLOW) {
        ok.mask = allow[(size_t)(blockIdx.x / W) * astride];
        bool any = false;
        if constexpr (STAGE) {
            for (int i = tid, k = 0; i < V; i += TW_TPB, ++k)
                ok.bits |= (unsigned long long)((ok.mask >> (word_cat[i] & 31)) & 1u) << k;
            any = ok.bits != 0;
            if (tid < r.head) r.row[tid] = r.g[tid];
            for (int j = tid; j < r.nvec; j += TW_TPB) *reinterpret_cast<float4*>(r.row + r.head + 4 * j) = r.g4[j];
            if (r.tail0 + tid < V) r.row[r.tail0 + tid] = r.g[r.tail0 + tid];
        } else {
            for (int i = tid; i < V; i += TW_TPB) any = any || ok(i);
        }
        const unsigned long long some = __ballot(any);
        if (lane == 0) any_w[wave] = some != 0 ? 1 : 0;
        __syncthreads();
        int found = 0;
#pragma unroll
        for (int k = 0; k < TW_WAVES; ++k) found |= any_w[k];
        if (!found) { ok.mask = 0xFFFFFFFFu; ok.bits = ~0ull; }
        float mx = -INFINITY;
        r.each([&](float x, int i) { if (ok(i)) mx = fmaxf(mx, x); });
        mx = wave_max(mx);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
#pragma unroll
        for (int k = 1; k < TW_WAVES; ++k) mx = fmaxf(mx, red[k]);
        __syncthreads();
        float s = 0.f;
        r.each([&](float x, int i) { if (ok(i)) s += __expf(x - mx); });
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < TW_WAVES; ++k) tot += red[k];
        lse = mx + logf(tot);
    } else {
        lse = r.stage_lse(red);
    }
    // ---- every entry's exact value; staged, its element of the row becomes the mark that leads to it
    if (tid < nslots) {
        float v = __uint_as_float(0x7FC00000u);
        if (mine >= 0) {
            float x;
            if constexpr (STAGE) x = r.row[mine]; else x = r.g[mine];
            v = x - lse;
            if constexpr (ALLOW) { if (!((ok.mask >> (word_cat[mine] & 31)) & 1u)) v -= 1000.0f; }
            if (mine == suppress) v -= 1000.0f;
            v -= 1000.0f;
        }
        bx[tid] = v;
        if constexpr (STAGE) { if (mine >= 0) r.row[mine] = __uint_as_float(0x7FC00000u | (unsigned)tid); }   // (distinct words: no two threads meet)
    }
    __syncthreads();
    const int lo = lo_s, hi = hi_s;
    auto val = [&](float x, int i) -> float {
        if constexpr (STAGE) {
            if (x != x) {
                const unsigned j = __float_as_uint(x) & 0x3FFFFFu;
                return j < (unsigned)nslots ? bx[j] : x;          // (a NaN of the row's own stays one: it ranks nowhere)
            }
        } else {
            if (i >= lo && i <= hi) {
                for (int j = 0; j < nslots; ++j) if (bw[j] == i) return bx[j];
            }
        }
        float v = x - lse;
        if constexpr (ALLOW) { if (!ok(i)) v -= 1000.0f; }
        if (i == suppress) v -= 1000.0f;
        return v;
    };
    // ---- the threshold selection of cap_beam_topw_thr_kernel over val
    float tm = -INFINITY;
    r.each([&](float x, int i) { tm = fmaxf(tm, val(x, i)); });
#pragma unroll
    for (int rd = 0; rd < W; ++rd) {
        const float m = wave_max(tm);
        const unsigned long long holders = __ballot(tm == m);
        if (lane == 0) cv[wave * W + rd] = m;
        if (holders != 0 && lane == __ffsll(holders) - 1) tm = -INFINITY;
    }
    __syncthreads();
    if (tid < TW_WAVES * W) {
        const float v = cv[tid];
        int rank = 0;
        for (int j = 0; j < TW_WAVES * W; ++j) {
            const float ov = cv[j];
            rank += (ov > v || (ov == v && j < tid)) ? 1 : 0;
        }
        if (rank == W - 1) tau_s = v;
    }
    __syncthreads();
    const float tau = tau_s;
    r.each([&](float x, int i) {
        const float v = val(x, i);
        if (v >= tau) {
            const int at = atomicAdd(&cnt_s, 1);
            if (at < TW_CAND) { lv[at] = v; li[at] = i; }
        }
    });
    __syncthreads();
    const int nc = cnt_s;
    if (nc < W || nc > TW_CAND) {                                 // uniform over the workgroup
        topw_by_insertion_of<W, STAGE>(r, val, cv, ci, topv, topi);
        return;
    }
    if (tid < nc) {
        const float v = lv[tid];
        const int ix = li[tid];
        int rank = 0;
        for (int j = 0; j < nc; ++j) rank += beam_before(lv[j], li[j], v, ix) ? 1 : 0;
        if (rank < W) {
            topv[(size_t)blockIdx.x * W + rank] = v;
            topi[(size_t)blockIdx.x * W + rank] = ix;             // (an index of `each`: inside [0, V))
        }
    }
}

template <int W, bool ALLOW>
int launch_topw_rules(hipStream_t st, const float* logits, int64_t ld, int M, int V, int suppress, const uint8_t* word_cat,
                      const uint32_t* allow, int64_t astride, const CapBeamBan& ban, float* topv, int32_t* topi) {
    const size_t row = ((size_t)V + 8) * sizeof(float), extra = 2 * ((size_t)ban.L + 1) * sizeof(int);
    if (row <= (size_t)CB_STAGE_BYTES) {                       // (the bound of the kernels without rules: the same form, the same sums)
        if (row + extra > 64 * 1024) {
            static std::atomic<unsigned> optin{0};
            XG_TRY(xg_lds_optin(optin, reinterpret_cast<const void*>(cap_beam_topw_rules_kernel<W, true, ALLOW>),
                                CB_STAGE_BYTES + RB_EXTRA_BYTES));
        }
        hipLaunchKernelGGL((cap_beam_topw_rules_kernel<W, true, ALLOW>), dim3(M), dim3(TW_TPB), row + extra, st, logits, ld, V, suppress,
                           word_cat, allow, astride, ban, V + 8, topv, topi);
    } else {
        hipLaunchKernelGGL((cap_beam_topw_rules_kernel<W, false, ALLOW>), dim3(M), dim3(TW_TPB), extra, st, logits, ld, V, suppress,
                           word_cat, allow, astride, ban, 0, topv, topi);
    }
    XG_CHECK_LAUNCH();
    return XG_OK;
}

template <int W>
int launch_topw_rules_any(hipStream_t st, const float* logits, int64_t ld, int M, int V, int suppress, const uint8_t* word_cat,
                          const uint32_t* allow, int64_t astride, const CapBeamBan& ban, float* topv, int32_t* topi) {
    return allow ? launch_topw_rules<W, true>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi)
                 : launch_topw_rules<W, false>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
}

template <int W, bool THR>
int launch_topw(hipStream_t st, const float* logits, int64_t ld, int M, int V, int suppress, float* topv, int32_t* topi) {
    using Kernel = void (*)(const float*, int64_t, int, int, float*, int32_t*);
    Kernel staged, unstaged;
    if constexpr (THR) { staged = cap_beam_topw_thr_kernel<W, true>; unstaged = cap_beam_topw_thr_kernel<W, false>; }
    else { staged = cap_beam_topw_kernel<W, true>; unstaged = cap_beam_topw_kernel<W, false>; }
    const size_t lds = ((size_t)V + 8) * sizeof(float);
    if (lds <= (size_t)CB_STAGE_BYTES) {
        if (lds > 64 * 1024) {                                 // > 64 KiB of dynamic LDS is opted into once per kernel and device
            static std::atomic<unsigned> optin{0};
            XG_TRY(xg_lds_optin(optin, reinterpret_cast<const void*>(staged), CB_STAGE_BYTES));
        }
        hipLaunchKernelGGL(staged, dim3(M), dim3(TW_TPB), lds, st, logits, ld, V, suppress, topv, topi);
    } else {
        hipLaunchKernelGGL(unstaged, dim3(M), dim3(TW_TPB), 0, st, logits, ld, V, suppress, topv, topi);
    }
    XG_CHECK_LAUNCH();
    return XG_OK;
}

template <bool THR>
int topw_any(hipStream_t st, const float* logits, int64_t ld, int M, int V, int W, int suppress, float* topv, int32_t* topi) {
    if (M <= 0 || V <= 0 || W < 1 || W > CB_MAX || W > V || ld < V || suppress >= V) return XG_EINVAL;
    if (suppress < 0) suppress = -1;
    switch (W) {
        case 1: return launch_topw<1, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 2: return launch_topw<2, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 3: return launch_topw<3, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 4: return launch_topw<4, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 5: return launch_topw<5, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 6: return launch_topw<6, THR>(st, logits, ld, M, V, suppress, topv, topi);
        case 7: return launch_topw<7, THR>(st, logits, ld, M, V, suppress, topv, topi);
        default: return launch_topw<8, THR>(st, logits, ld, M, V, suppress, topv, topi);
    }
}

__global__ void __launch_bounds__(CB_TPB) cap_beam_merge_kernel(CapBeamMergeArgs a) {
    __shared__ BeamTables T;
    const int tid = threadIdx.x;
    const int R = a.R, W = a.book.W;
    const size_t b = blockIdx.x, row0 = b * W;
    const int rows = a.book.t == 0 ? 1 : W;   // (every slot holds the video's initial state at t = 0)
    if (tid < CB_MAX * CB_MAX) {              // (whatever topw left unwritten is word 0, never an index out of range)
        const int q = tid / CB_MAX, k = tid - q * CB_MAX;
        float lp = 0.f;
        int tk = 0;
        if (q < rows && k < W) {
            lp = a.topv[(row0 + q) * W + k];
            tk = a.topi[(row0 + q) * W + k];
            tk = tk < 0 ? 0 : (tk >= a.V ? a.V - 1 : tk);
        }
        T.c_lp[tid] = lp; T.c_tok[tid] = tk;
    }
    beam_merge(T, a.book, b, rows);
    // slot v takes h1, c1, h2, c2 of its parent: out of the buffer the step wrote, into the buffer the next step reads
    if (a.vec) {
        const int R4 = R >> 2;
        for (int i = tid; i < 4 * W * R4; i += CB_TPB) {
            const int k = i / (W * R4), rem = i - k * (W * R4);
            const int v = rem / R4, j = rem - v * R4;
            reinterpret_cast<float4*>(a.dst[k] + (row0 + v) * R)[j] = reinterpret_cast<const float4*>(a.src[k] + (row0 + T.s_q[v]) * R)[j];
        }
    } else {
        for (int i = tid; i < 4 * W * R; i += CB_TPB) {
            const int k = i / (W * R), rem = i - k * (W * R);
            const int v = rem / R, j = rem - v * R;
            a.dst[k][(row0 + v) * R + j] = a.src[k][(row0 + T.s_q[v]) * R + j];
        }
    }
    // under rules slot v's history is its parent's t tokens and, appended, its own
    if (a.hdst) {
        const int t = a.book.t, L = a.book.L;
        for (int i = tid; i < W * (t + 1); i += CB_TPB) {
            const int v = i / (t + 1), j = i - v * (t + 1);
            a.hdst[(row0 + v) * L + j] = j < t ? a.hsrc[(row0 + T.s_q[v]) * L + j] : T.s_tok[v];
        }
    }
}

// one thread per (video, rank): the done entry's beam, read back along its parents
__global__ void __launch_bounds__(CB_TPB) cap_beam_backtrace_kernel(BeamBook<int64_t> k, int64_t* seq, float* seq_logp, float* score,
                                                                    int M) {
    const int i = blockIdx.x * CB_TPB + threadIdx.x;
    if (i < M) beam_backtrace_row(k, i, seq, seq_logp, score);
}

// dst row b W + slot = src row b, for every entry in one launch (blockIdx.y: the entry)
__global__ void __launch_bounds__(CB_TPB) cap_beam_repeat_kernel(CapBeamRepeatArgs a, int B, int W) {
    const CapBeamRepeatEntry e = a.e[blockIdx.y];
    const int64_t n = e.n, total = (int64_t)B * W * n;
    const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(e.dst) | reinterpret_cast<uintptr_t>(e.src)) % 16 == 0);
    const int64_t step = (int64_t)gridDim.x * CB_TPB;
    if (vec) {
        for (int64_t i = ((int64_t)blockIdx.x * CB_TPB + threadIdx.x) * 4; i < total; i += step * 4) {
            const int64_t m = i / n, j = i - m * n;
            *reinterpret_cast<float4*>(e.dst + i) = *reinterpret_cast<const float4*>(e.src + (m / W) * n + j);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * CB_TPB + threadIdx.x; i < total; i += step) {
            const int64_t m = i / n, j = i - m * n;
            e.dst[i] = e.src[(m / W) * n + j];
        }
    }
}

}  // namespace

int xgk_cap_beam_repeat(hipStream_t st, const CapBeamRepeatArgs& a, int B, int W) {
    if (a.n <= 0 || a.n > XG_CAP_BEAM_REPEAT_MAX || B <= 0 || W <= 0) return XG_EINVAL;
    int64_t most = 0;
    for (int i = 0; i < a.n; ++i) {
        if (!a.e[i].dst || !a.e[i].src || a.e[i].n <= 0) return XG_EINVAL;
        most = a.e[i].n > most ? a.e[i].n : most;
    }
    const int64_t blocks = xg_cdiv64((int64_t)B * W * most, (int64_t)CB_TPB * 4);
    hipLaunchKernelGGL(cap_beam_repeat_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048), a.n), dim3(CB_TPB), 0, st, a, B, W);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_cap_beam_topw(hipStream_t st, const float* logits, int64_t ld, int M, int V, int W, int suppress, float* topv, int32_t* topi) {
    return topw_any<false>(st, logits, ld, M, V, W, suppress, topv, topi);
}

int xgk_cap_beam_topw_thr(hipStream_t st, const float* logits, int64_t ld, int M, int V, int W, int suppress, float* topv, int32_t* topi) {
    return topw_any<true>(st, logits, ld, M, V, W, suppress, topv, topi);
}

int xgk_cap_beam_topw_allow(hipStream_t st, const float* logits, int64_t ld, int M, int V, int W, int suppress, const uint8_t* word_cat,
                            const uint32_t* allow, int64_t astride, float* topv, int32_t* topi) {
    if (M <= 0 || V <= 0 || W < 1 || W > CB_MAX || W > V || ld < V || suppress >= V || !word_cat || !allow || astride < 1 || M % W)
        return XG_EINVAL;
    if (suppress < 0) suppress = -1;
    switch (W) {
        case 1: return launch_topw_allow<1>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 2: return launch_topw_allow<2>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 3: return launch_topw_allow<3>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 4: return launch_topw_allow<4>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 5: return launch_topw_allow<5>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 6: return launch_topw_allow<6>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        case 7: return launch_topw_allow<7>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
        default: return launch_topw_allow<8>(st, logits, ld, M, V, suppress, word_cat, allow, astride, topv, topi);
    }
}

int xgk_cap_beam_topw_rules(hipStream_t st, const float* logits, int64_t ld, int M, int V, int W, int suppress, const uint8_t* word_cat,
                            const uint32_t* allow, int64_t astride, const CapBeamBan& ban, float* topv, int32_t* topi) {
    if (M <= 0 || V <= 0 || W < 1 || W > CB_MAX || W > V || ld < V || suppress >= V || !word_cat != !allow || astride < 1 || M % W)
        return XG_EINVAL;
    if (!ban.hist || ban.L < 1 || ban.L > RB_LMAX || ban.t < 0 || ban.t >= ban.L || ban.ngram < 0 || ban.min_length < 0 ||
        ban.n_bad_end < 0 || ban.n_bad_end > XGBR_MAX_BAD_END || (ban.n_bad_end > 0 && !ban.bad_end))
        return XG_EINVAL;
    if (suppress < 0) suppress = -1;
    switch (W) {
        case 1: return launch_topw_rules_any<1>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 2: return launch_topw_rules_any<2>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 3: return launch_topw_rules_any<3>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 4: return launch_topw_rules_any<4>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 5: return launch_topw_rules_any<5>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 6: return launch_topw_rules_any<6>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        case 7: return launch_topw_rules_any<7>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
        default: return launch_topw_rules_any<8>(st, logits, ld, M, V, suppress, word_cat, allow, astride, ban, topv, topi);
    }
}

int xgk_cap_beam_merge(hipStream_t st, int B, CapBeamMergeArgs a) {
    const BeamBook<int64_t>& k = a.book;
    if (B <= 0 || k.W < 1 || k.W > CB_MAX || a.R <= 0 || k.L <= 0 || k.t < 0 || k.t >= k.L) return XG_EINVAL;
    if ((a.hdst && !a.hsrc) || (k.scale && !k.done_key)) return XG_EINVAL;
    uintptr_t bits = 0;
    for (int k = 0; k < 4; ++k) bits |= reinterpret_cast<uintptr_t>(a.src[k]) | reinterpret_cast<uintptr_t>(a.dst[k]);
    a.vec = (a.R % 4 == 0 && bits % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(cap_beam_merge_kernel, dim3(B), dim3(CB_TPB), 0, st, a);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_cap_beam_backtrace(hipStream_t st, int B, const BeamBook<int64_t>& book, int64_t* seq, float* seq_logp, float* score) {
    const int M = B * book.W;
    hipLaunchKernelGGL(cap_beam_backtrace_kernel, dim3(xg_cdiv(M, CB_TPB)), dim3(CB_TPB), 0, st, book, seq, seq_logp, score, M);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// ---- the diverse search (include/xgate_beam_diverse.h): a pair's N = Gd Wg rows hold their N best words each (topv / topi (M,N), the
// selection kernel at W = N; a row's Wg best PENALISED words lie inside its unpenalised top N, docs/CAPTION_DIVERSE.md).  One
// workgroup per pair, the groups in series: each row of group j is re-ranked under the penalty of the earlier groups' live new
// words, beam_group_merge commits the group into the book carved as (pairs Gd, Wg, L), then every thread gathers slot v's state
// from its parent row of the pair.
namespace {

__global__ void __launch_bounds__(CB_TPB) cap_beam_merge_diverse_kernel(CapBeamMergeArgs a, int Gd, float lambda) {
    __shared__ BeamGroupTables G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, Wg = a.book.W, N = Gd * Wg;
    const size_t pair = blockIdx.x, row0 = pair * N;
    const int rows = a.book.t == 0 ? 1 : Wg;  // (every slot holds the video's initial state at t = 0: a group's first row stands for it)
    beam_group_begin(G);
    for (int j = 0; j < Gd; ++j) {
        for (int q = wave; q < rows; q += CB_TPB / 64) {
            const size_t at = (row0 + (size_t)j * Wg + q) * N;
            beam_group_rerank(G, q, a.topv + at, a.topi + at, N, a.V - 1, Wg, lambda, lane);
        }
        beam_group_merge(G, a.book, pair, Gd, j, rows);
    }
    if (a.vec) {
        const int R4 = R >> 2;
        for (int i = tid; i < 4 * N * R4; i += CB_TPB) {
            const int k = i / (N * R4), rem = i - k * (N * R4);
            const int v = rem / R4, j = rem - v * R4;
            reinterpret_cast<float4*>(a.dst[k] + (row0 + v) * R)[j] = reinterpret_cast<const float4*>(a.src[k] + (row0 + G.par[v]) * R)[j];
        }
    } else {
        for (int i = tid; i < 4 * N * R; i += CB_TPB) {
            const int k = i / (N * R), rem = i - k * (N * R);
            const int v = rem / R, j = rem - v * R;
            a.dst[k][(row0 + v) * R + j] = a.src[k][(row0 + G.par[v]) * R + j];
        }
    }
}

}  // namespace

int xgk_cap_beam_merge_diverse(hipStream_t st, int pairs, CapBeamMergeArgs a, int Gd, float lambda) {
    const BeamBook<int64_t>& k = a.book;
    if (pairs <= 0 || Gd < 1 || Gd > CB_MAX || k.W < 1 || k.W > CB_MAX || Gd * k.W > CB_MAX || Gd * k.W > a.V || a.R <= 0 || k.L <= 0 ||
        k.t < 0 || k.t >= k.L || !(lambda >= 0.0f) || lambda == INFINITY)
        return XG_EINVAL;
    uintptr_t bits = 0;
    for (int i = 0; i < 4; ++i) bits |= reinterpret_cast<uintptr_t>(a.src[i]) | reinterpret_cast<uintptr_t>(a.dst[i]);
    a.vec = (a.R % 4 == 0 && bits % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(cap_beam_merge_diverse_kernel, dim3(pairs), dim3(CB_TPB), 0, st, a, Gd, lambda);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
