// Scoring GIVEN captions (include/xgate_score.h): what a row's hidden state says about ONE known token per step.
//
// Of the (rows, V) logits x = h2' W_logit^T + b a scored row needs two numbers: its log-sum-exp and the logit of its target.  The
// kernels below produce both and the logits never touch memory:
//
//   score_part_kernel   128 rows x 32 vocabulary columns per workgroup (4 waves, one 32 x 32 fp32 MFMA tile each, the W slab shared:
//                       the loop of xg_heads.hip's vocab_part_kernel) for ANY number of rows -- grid (vocabulary tiles, row tiles of
//                       128, the last one partial).  Epilogue: per (row, tile) the max and sum exp(x - max) over the tile's columns
//                       (columns past V are -inf), and the target's logit from the ONE tile that owns the target column.
//   score_rows_kernel   every other shape (R no multiple of 32, V < 32, unaligned operands): one workgroup per row, a thread per
//                       column, an online max-shifted sum per thread, one tree merge in a fixed order.  One "tile" per row.
//   score_reduce_kernel per (row, step of the chunk) the max over the tiles, then the sum of the tiles' sums shifted to it, and
//                       tok_logp = target logit - LSE masked by the counted columns.
//   score_sum_kernel    behind the last chunk: a row's score, its tok_logp added in column order.
//
// Every exponential is max-shifted (a raw logit past 88.7 overflows exp in fp32).  No float atomics: every number has one writer and
// every sum one fixed order, so a result depends neither on the order in which workgroups finish nor on the chunking's timing.
#include "xg_common.h"
#include "xg_kernels.h"

namespace {

typedef float s_f32x16 __attribute__((ext_vector_type(16)));
typedef float s_f32x4 __attribute__((ext_vector_type(4)));
typedef float s_f32x2 __attribute__((ext_vector_type(2)));
constexpr int SC_LD = 36;                 // LDS row stride of a 32-deep slab (floats): conflict-free b128 fragment reads
constexpr int SC_ROWS = 128;              // rows per workgroup
constexpr int SC_TW = XGK_SCORE_TILE;     // vocabulary columns per workgroup

struct ScoreArgs {
    const float* H;                       // (rows, R)
    const float* W; const float* bias;    // (V, R) row-major, (V)
    const int32_t* tgt;                   // (rows) target column, in [0, V)
    float* part;                          // (ntiles, rows, 2): max, sum exp(x - max)
    float* tlogit;                        // (rows)
    int rows, R, V;
};

__global__ void __launch_bounds__(256) score_part_kernel(ScoreArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * (SC_ROWS + SC_TW) * SC_LD];
    constexpr int STAGE = (SC_ROWS + SC_TW) * SC_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int n0 = blockIdx.x * SC_TW, r0 = blockIdx.y * SC_ROWS;
    // per-thread load pieces of a slab: A 128 x 32 -> 4 float4 (row f >> 3, k (f & 7) * 4), W 32 x 32 -> 1 float4.  Rows past the
    // last one and columns past V read the last valid row again: in bounds, and what they compute is never stored.
    const float* ap[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = tid + 256 * i;
        ap[i] = a.H + (size_t)min(r0 + (f >> 3), a.rows - 1) * a.R + ((f & 7) << 2);
    }
    const float* wp = a.W + (size_t)min(n0 + (tid >> 3), a.V - 1) * a.R + ((tid & 7) << 2);
    s_f32x4 ra[2][4], rw[2];              // global loads run two slabs ahead of their MFMAs (two register sets)
    auto ld = [&](int s, s_f32x4 (&xa)[4], s_f32x4& xw) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xa[i] = *reinterpret_cast<const s_f32x4*>(ap[i] + s * 32);
        xw = *reinterpret_cast<const s_f32x4*>(wp + s * 32);
    };
    auto st = [&](int buf, const s_f32x4 (&xa)[4], const s_f32x4& xw) {
        float* As = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = tid + 256 * i;
            *reinterpret_cast<s_f32x4*>(As + (f >> 3) * SC_LD + ((f & 7) << 2)) = xa[i];
        }
        *reinterpret_cast<s_f32x4*>(As + SC_ROWS * SC_LD + (tid >> 3) * SC_LD + ((tid & 7) << 2)) = xw;
    };
    s_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ns = a.R / 32;
    ld(0, ra[0], rw[0]);
    if (ns > 1) ld(1, ra[1], rw[1]);
    st(0, ra[0], rw[0]);
    __syncthreads();
    auto slab = [&](int s, s_f32x4 (&mine)[4], s_f32x4& minew, const s_f32x4 (&other)[4], const s_f32x4& otherw) {
        if (s + 2 < ns) ld(s + 2, mine, minew);          // (this set's slab s is in LDS)
        const float* As = smem + (s & 1) * STAGE;
        const float* Bs = As + SC_ROWS * SC_LD;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const s_f32x4 fa = *reinterpret_cast<const s_f32x4*>(As + (wave * 32 + l31) * SC_LD + kb * 8 + half * 4);
            const s_f32x4 fb = *reinterpret_cast<const s_f32x4*>(Bs + l31 * SC_LD + kb * 8 + half * 4);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[kk], acc, 0, 0, 0);
        }
        if (s + 1 < ns) st((s + 1) & 1, other, otherw);   // slab s + 1: requested two slabs ago
        __syncthreads();
    };
    for (int s = 0; s < ns; s += 2) {
        slab(s, ra[0], rw[0], ra[1], rw[1]);
        if (s + 1 < ns) slab(s + 1, ra[1], rw[1], ra[0], rw[0]);
    }
    // epilogue through LDS (the staging buffers are free: every wave is past the loop's last barrier): the tile as [128][33], then
    // thread (row, half-row) walks 16 columns and exchanges with its neighbour
    constexpr int TL = 33;
    float* tl = smem;
    {
        const int col = n0 + l31;
        const float bv = col < a.V ? a.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) tl[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * TL + l31] = acc[r] + bv;
    }
    __syncthreads();
    const int row = tid >> 1, h = tid & 1, c0 = n0 + h * 16, grow = r0 + row;
    const bool live = grow < a.rows;
    const int tcol = (live ? a.tgt[grow] : -1) - c0;          // the target's place among this thread's 16 columns, if it is one of them
    float x[16];
    float m = -INFINITY, tx = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        x[j] = c0 + j < a.V ? tl[row * TL + h * 16 + j] : -INFINITY;
        m = fmaxf(m, x[j]);
        if (j == tcol) tx = x[j];
    }
    m = fmaxf(m, __shfl_xor(m, 1, 64));                       // (column n0 is below V: the pair's max is finite)
    float e1 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) e1 += __expf(x[j] - m);      // (-inf for columns past V: exp -> 0)
    e1 += __shfl_xor(e1, 1, 64);
    if (live) {
        if (h == 0) {
            const s_f32x2 pv = {m, e1};
            *reinterpret_cast<s_f32x2*>(a.part + ((size_t)blockIdx.x * a.rows + grow) * 2) = pv;
        }
        if (tcol >= 0 && tcol < 16) a.tlogit[grow] = tx;
    }
}

constexpr int SR_T = 256;
// (m, s) <- (m, s) merged with (m2, s2): both sums shifted to the common max; an empty side (-inf, 0) leaves the other unchanged
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) return;
    s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
    m = mm;
}

__global__ void __launch_bounds__(SR_T) score_rows_kernel(ScoreArgs a) {
    __shared__ float sm[SR_T], ss[SR_T];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* h = a.H + (size_t)row * a.R;
    const int t = a.tgt[row];
    float m = -INFINITY, s = 0.f;
    for (int v = tid; v < a.V; v += SR_T) {
        const float* w = a.W + (size_t)v * a.R;
        float x = a.bias[v];
        for (int k = 0; k < a.R; ++k) x = fmaf(h[k], w[k], x);
        if (v == t) a.tlogit[row] = x;
        lse_merge(m, s, x, 1.0f);
    }
    sm[tid] = m; ss[tid] = s;
    __syncthreads();
    for (int w = SR_T / 2; w > 0; w >>= 1) {
        if (tid < w) {
            lse_merge(m, s, sm[tid + w], ss[tid + w]);
            sm[tid] = m; ss[tid] = s;
        }
        __syncthreads();
    }
    if (tid == 0) { a.part[(size_t)row * 2] = m; a.part[(size_t)row * 2 + 1] = s; }
}

// block (16 rows, 16 tile lanes) of one step of the chunk: thread (r, l) walks tiles l, l + 16, ... of its row -- a wave's load is
// four 128-byte pieces of four tiles' row arrays --, first for the max, then for the sums shifted to it; the 16 lanes of a row meet in
// LDS and are added in lane order
constexpr int RD_ROWS = 16, RD_LANES = 16;
__global__ void __launch_bounds__(RD_ROWS * RD_LANES) score_reduce_kernel(const float* __restrict__ part, const float* __restrict__ tlogit,
                                                                          int ntiles, int M, int L, int step0, int steps,
                                                                          const int32_t* __restrict__ count, float* __restrict__ tok_logp) {
    __shared__ float red[RD_LANES][RD_ROWS + 1];
    const int r = threadIdx.x & (RD_ROWS - 1), l = threadIdx.x / RD_ROWS, s = blockIdx.y;
    const int m = min(blockIdx.x * RD_ROWS + r, M - 1);           // (rows past the last one repeat it and store nothing)
    const size_t nrows = (size_t)steps * M, cr = (size_t)s * M + m;
    const s_f32x2* pr = reinterpret_cast<const s_f32x2*>(part) + cr;
    float mx = -INFINITY;
    for (int t = l; t < ntiles; t += RD_LANES) mx = fmaxf(mx, pr[(size_t)t * nrows][0]);
    red[l][r] = mx;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RD_LANES; ++i) mx = fmaxf(mx, red[i][r]);
    __syncthreads();
    float sum = 0.f;
    for (int t = l; t < ntiles; t += RD_LANES) {
        const s_f32x2 v = pr[(size_t)t * nrows];
        sum += v[1] * __expf(v[0] - mx);
    }
    red[l][r] = sum;
    __syncthreads();
    if (l == 0 && blockIdx.x * RD_ROWS + r < M) {
        sum = 0.f;
#pragma unroll
        for (int i = 0; i < RD_LANES; ++i) sum += red[i][r];
        const int j = step0 + s;
        tok_logp[(size_t)m * L + j] = j < count[m] ? tlogit[cr] - (mx + logf(sum)) : 0.f;
    }
}

// score = the sum of a row's tok_logp in column order (uncounted columns hold 0)
__global__ void __launch_bounds__(256) score_sum_kernel(const float* __restrict__ tok_logp, int M, int L, float* __restrict__ score) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float acc = 0.f;
    for (int j = 0; j < L; ++j) acc += tok_logp[(size_t)m * L + j];
    score[m] = acc;
}

__global__ void __launch_bounds__(256) score_prep_kernel(const int64_t* __restrict__ tokens, int M, int L, int V, int64_t* __restrict__ fed,
                                                         int32_t* __restrict__ tgt, float* __restrict__ unf, int32_t* __restrict__ count) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int64_t prev = 0;                     // BOS
    bool alive = true;
    int cnt = 0;
    for (int j = 0; j < L; ++j) {
        const size_t o = (size_t)j * M + m;
        if (j > 0) alive = alive && prev > 0;
        cnt += alive ? 1 : 0;
        int64_t tk = tokens[(size_t)m * L + j];
        tk = tk < 0 ? 0 : (tk >= V ? V - 1 : tk);
        fed[o] = prev; tgt[o] = (int32_t)tk; unf[o] = alive ? 1.0f : 0.0f;
        prev = tk;
    }
    count[m] = cnt;
}

inline bool score_fast(int R, int V, const float* H, const float* W) {
    return R % 32 == 0 && V >= SC_TW && (reinterpret_cast<uintptr_t>(H) % 16 == 0) && (reinterpret_cast<uintptr_t>(W) % 16 == 0);
}

}  // namespace

int xgk_score_prep(hipStream_t st, const int64_t* tokens, int M, int L, int V, int64_t* fed, int32_t* tgt, float* unf, int32_t* count) {
    hipLaunchKernelGGL(score_prep_kernel, dim3(xg_cdiv(M, 256)), dim3(256), 0, st, tokens, M, L, V, fed, tgt, unf, count);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_score_tiles(int R, int V, const float* H, const float* W) { return score_fast(R, V, H, W) ? xg_cdiv(V, SC_TW) : 1; }

int xgk_score_part(hipStream_t st, int rows, int R, int V, const float* H, const float* W, const float* bias, const int32_t* tgt,
                   float* part, float* tlogit) {
    if (rows < 1 || R < 1 || V < 1) return XG_EINVAL;
    const ScoreArgs a{H, W, bias, tgt, part, tlogit, rows, R, V};
    if (score_fast(R, V, H, W)) {
        if (xg_cdiv(rows, SC_ROWS) > 65535) return XG_EINVAL;
        hipLaunchKernelGGL(score_part_kernel, dim3(xg_cdiv(V, SC_TW), xg_cdiv(rows, SC_ROWS)), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(score_rows_kernel, dim3(rows), dim3(SR_T), 0, st, a);
    }
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_score_reduce(hipStream_t st, const float* part, const float* tlogit, int ntiles, int M, int L, int step0, int steps,
                     const int32_t* count, float* tok_logp) {
    if (steps < 1 || steps > 65535) return XG_EINVAL;
    hipLaunchKernelGGL(score_reduce_kernel, dim3(xg_cdiv(M, RD_ROWS), steps), dim3(RD_ROWS * RD_LANES), 0, st, part, tlogit, ntiles, M,
                       L, step0, steps, count, tok_logp);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

int xgk_score_sum(hipStream_t st, const float* tok_logp, int M, int L, float* score) {
    hipLaunchKernelGGL(score_sum_kernel, dim3(xg_cdiv(M, 256)), dim3(256), 0, st, tok_logp, M, L, score);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
