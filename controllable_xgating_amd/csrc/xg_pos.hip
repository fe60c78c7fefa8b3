// POS sequence generator (reference pos_src/SAModel.py, pos_src/sub_modules.py): eval-mode inference behind include/xgate_pos.h.
//
// The model is a strict subset of the captioner: the same Linear -> BN -> ReLU embeddings, two masked LSTMCell encoders and the
// late fusion (no cross gates), a ONE-layer attention decoder and a C-way category head.  The encoder and every product reuse the
// captioner's launchers (xg_kernels.h) unchanged; what is new here is the decoder step:
//   1. p = h2a(h)                        xgk_skinny, one job               (B, A)
//   2. attention over the hoisted v2a(V)   pos_attn_kernel                 af -> X[:, 0:R]
//   3. af a2h^T + h h2h^T                 xgk_skinny, one job of two segments (B, 4R)
//   4. cell epilogue + category head      pos_cell_head_kernel: i2h(embed[tok]) is a row of the (C, 4R) table embed i2h^T + b
//      hoisted once per call; the cell writes h' into X[:, R:2R] (the next step's input) and the state row of the step, then the
//      same workgroup computes the C logits, log_softmax, the greedy choice and the `unfinished` / mask bookkeeping of its video.
// All steps run on the device; the reference's early exits (teacher forcing: an all-zero category column; greedy: every row
// finished) are computed afterwards by pos_first_zero_col_kernel into a device word, so a call never synchronises with the host.
#include "xg_kernels.h"
#include "../../include/xgate_pos.h"

namespace {

constexpr int POS_TPB = 256;
// the two per-video kernels of the step run 16 waves per workgroup: the step has only B workgroups, and each of them is bound by
// the latency of its loads (the hoisted v2a(V) rows, V, the weight rows of the head), so more waves keep more loads in flight
// (256-thread versions took 34 and 15 us per step at B = 64, K = 20)
constexpr int STEP_TPB = 1024;
constexpr int STEP_WAVES = STEP_TPB / 64;
__device__ __forceinline__ int xg_cdiv_d(int a, int b) { return (a + b - 1) / b; }

// one workgroup per video: e_k = w . tanh(p + q_k) (one wave per frame at a time), alpha = softmax_k(e) over ALL K frames
// (pos_src/sub_modules.py:701-708: the softmax is not masked; a2w.bias cancels in it), af = sum_k alpha_k V_k into X[b, 0:R].
// The context sums run in `nsplit` interleaved parts over the frames, added in part order: every element has one fixed order.
template <bool V4>
__global__ void __launch_bounds__(STEP_TPB) pos_attn_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const float* __restrict__ V, const float* __restrict__ w, float* X, int K,
                                                            int R, int A, int nsplit) {
    extern __shared__ float lds[];
    float* ps = lds;              // A
    float* wsh = lds + A;         // A
    float* al = lds + 2 * A;      // K
    float* red = al + K;          // nsplit * R
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vb = V + (size_t)b * K * R;
    // the context's V operands are requested first (they do not depend on the scores): one latency round instead of two
    constexpr int VREG = 16;
    const bool vpre = nsplit * R <= STEP_TPB && xg_cdiv_d(K, nsplit) <= VREG;
    const int vr = tid % R, vpart = tid / R;
    float vreg[VREG];
    if (vpre && tid < nsplit * R) {
#pragma unroll
        for (int i = 0; i < VREG; ++i) {
            const int k = vpart + i * nsplit;
            vreg[i] = k < K ? vb[(size_t)k * R + vr] : 0.f;
        }
    }
    for (int a = tid; a < A; a += STEP_TPB) {
        ps[a] = P[(size_t)b * A + a];
        wsh[a] = w[a];
    }
    __syncthreads();
    // frames k0 and k0 + 16 of a wave together, so that both rows of v2a(V) are in flight at once
    for (int k0 = wave; k0 < K; k0 += 2 * STEP_WAVES) {
        const int k1 = k0 + STEP_WAVES;
        const bool two = k1 < K;                                // wave-uniform
        const float* q0 = Q + ((size_t)b * K + k0) * A;
        const float* q1 = Q + ((size_t)b * K + (two ? k1 : k0)) * A;
        float acc0 = 0.f, acc1 = 0.f;
        if (V4) {
            const float4* q04 = reinterpret_cast<const float4*>(q0);
            const float4* q14 = reinterpret_cast<const float4*>(q1);
#pragma unroll 6
            for (int a4 = lane; a4 < A / 4; a4 += 64) {
                const float4 u = q04[a4];
                const float4 v = q14[a4];
                const int a = 4 * a4;
                const float p0 = ps[a], p1 = ps[a + 1], p2 = ps[a + 2], p3 = ps[a + 3];
                const float w0 = wsh[a], w1 = wsh[a + 1], w2 = wsh[a + 2], w3 = wsh[a + 3];
                acc0 += w0 * xg_tanh(p0 + u.x) + w1 * xg_tanh(p1 + u.y) + w2 * xg_tanh(p2 + u.z) + w3 * xg_tanh(p3 + u.w);
                acc1 += w0 * xg_tanh(p0 + v.x) + w1 * xg_tanh(p1 + v.y) + w2 * xg_tanh(p2 + v.z) + w3 * xg_tanh(p3 + v.w);
            }
        } else {
#pragma unroll 4
            for (int a = lane; a < A; a += 64) {
                const float u = q0[a], v = q1[a];
                acc0 += wsh[a] * xg_tanh(ps[a] + u);
                acc1 += wsh[a] * xg_tanh(ps[a] + v);
            }
        }
        acc0 = wave_sum(acc0);
        acc1 = wave_sum(acc1);
        if (lane == 0) {
            al[k0] = acc0;
            if (two) al[k1] = acc1;
        }
    }
    __syncthreads();
    float mx = al[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, al[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += __expf(al[k] - mx);
    __syncthreads();                                           // (every thread has read the scores)
    for (int k = tid; k < K; k += STEP_TPB) al[k] = __expf(al[k] - mx) / s;
    __syncthreads();
    if (vpre) {
        if (tid < nsplit * R) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < VREG; ++i) {
                const int k = vpart + i * nsplit;
                if (k < K) acc += al[k] * vreg[i];
            }
            red[tid] = acc;
        }
    } else {
        for (int i = tid; i < nsplit * R; i += STEP_TPB) {
            const int r = i % R, part = i / R;
            float acc = 0.f;
#pragma unroll 4
            for (int k = part; k < K; k += nsplit) acc += al[k] * vb[(size_t)k * R + r];
            red[i] = acc;
        }
    }
    __syncthreads();
    for (int r = tid; r < R; r += STEP_TPB) {
        float acc = red[r];
        for (int part = 1; part < nsplit; ++part) acc += red[part * R + r];
        X[(size_t)b * 2 * R + r] = acc;
    }
}

// A (N,K) row-major weight re-tiled for the skinny launcher's fast kernel (SkSeg.Bp: 32 x 32 tiles, nck = ceil(K/32) tiles per 32-row
// slice, each tile in the MFMA-fragment order [i(4)][h(2)][n(32)][q(4)] -> element (n, 16 h + 4 i + q) that xg_pack.hip writes for
// its fp32 shadow).  One workgroup per tile; zero padding past N and K.
__global__ void __launch_bounds__(POS_TPB) pos_pack_kernel(const float* __restrict__ src, int N, int K, float* __restrict__ dst) {
    __shared__ float t[32][33];
    const int nck = (K + 31) >> 5;
    const int tile = blockIdx.x, tn = tile / nck, kc = tile - tn * nck;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = ty + 8 * r, n = tn * 32 + nn, k = kc * 32 + tx;
        t[nn][tx] = (n < N && k < K) ? src[(size_t)n * K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = threadIdx.x + POS_TPB * r;
        const int q = o & 3, nn = (o >> 2) & 31, h = (o >> 7) & 1, i = o >> 8;
        dst[(size_t)tile * 1024 + o] = t[nn][16 * h + 4 * i + q];
    }
}

inline size_t packed_floats(int N, int K) { return (size_t)xg_cdiv(N, 32) * xg_cdiv(K, 32) * 1024; }

// tab (C,4R) += a2h.bias + h2h.bias: the per-step cell then adds ONE hoisted row per video
__global__ void __launch_bounds__(POS_TPB) pos_fold_bias_kernel(float* tab, const float* b1, const float* b2, int C, int N) {
    const int64_t i = (int64_t)blockIdx.x * POS_TPB + threadIdx.x;
    if (i >= (int64_t)C * N) return;
    const int n = (int)(i % N);
    tab[i] += b1[n] + b2[n];
}

struct CellHeadArgs {
    const float* S;              // (B,4R) af a2h^T + h h2h^T, no bias
    const float* tab;            // (C,4R) embed i2h^T + i2h.bias + a2h.bias + h2h.bias
    const float *logit_w, *logit_b;
    float* X;                    // (B,2R): h read from and h' written to columns R..2R
    float* c;                    // (B,R) cell state, in place
    int B, R, C, T, t;
    // teacher forcing: tokens and masks of the step from the (B,T) inputs, logp (B,T,C) out
    const int64_t* cap; const float* new_mask; float* logp;
    // greedy: tok (B) = the previous step's choice, masks (B,T), seq / seq_logp (B,T-1), states (B,T,R)
    int64_t* tok; float* masks; int64_t* seq; float* seq_logp; float* states;
};

// the greedy choice of step t + 1 from the log-probabilities of step t (SAModel.py:142-166): torch.max's first maximum, then
// `unfinished`, the masked token, its log-prob and the next step's mask
__device__ __forceinline__ void pos_choose(const CellHeadArgs& a, int b, int best, float bv) {
    const size_t T = a.T;
    const float unf_prev = a.t == 0 ? 1.0f : a.masks[b * T + a.t];
    const float unf = best > 0 ? unf_prev : 0.0f;
    a.seq[b * (T - 1) + a.t] = unf != 0.0f ? best : 0;
    a.seq_logp[b * (T - 1) + a.t] = bv;
    a.masks[b * T + a.t + 1] = unf;
    a.tok[b] = best;
}

// The straight-line pieces every cell-head kernel of this file shares (greedy / teacher-forced, train, rows).  The greedy, forced and
// sampled calls are bit-identical where they meet (tested) BECAUSE these are one definition each: hipcc contracts to FMA, so a
// regrouped expression here changes bits everywhere at once, never in one kernel alone.

// (the reference would raise on an out-of-range category)
__device__ __forceinline__ int64_t pos_clamp_tag(int64_t tk, int C) { return tk < 0 ? 0 : (tk >= C ? C - 1 : tk); }

// unit j of the two_inputs_lstmcell epilogue (pos_src/sub_modules.py:871-889: order i,f,o,g, the mask holds c and h) from the row
// s of the step's product, the hoisted token row tb and the state (cp, hp) before the step
struct PosCell { float ig, fg, og, gg, cn, hn; };   // the activated gates and the new state, held where the mask is 0
__device__ __forceinline__ PosCell pos_cell(const float* s, const float* tb, int R, int j, float cp, float hp, float m) {
    PosCell o;
    o.ig = xg_sigmoid(s[j] + tb[j]), o.fg = xg_sigmoid(s[R + j] + tb[R + j]);
    o.og = xg_sigmoid(s[2 * R + j] + tb[2 * R + j]), o.gg = xg_tanh(s[3 * R + j] + tb[3 * R + j]);
    o.cn = o.fg * cp + o.ig * o.gg;
    o.cn = o.cn * m + cp * (1.0f - m);
    o.hn = o.og * xg_tanh(o.cn);
    o.hn = o.hn * m + hp * (1.0f - m);
    return o;
}

// lg[0:C] = logit_w hs + logit_b, one wave per category at a time.  Called by the whole workgroup: the first barrier makes hs
// (written by the cell loop) visible, the second lg.
__device__ __forceinline__ void pos_head_logits(const float* logit_w, const float* logit_b, const float* hs, float* lg, int R, int C) {
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int cc = wave; cc < C; cc += STEP_WAVES) {
        const float* wr = logit_w + (size_t)cc * R;
        float acc = 0.f;
#pragma unroll 8
        for (int j = lane; j < R; j += 64) acc += wr[j] * hs[j];
        acc = wave_sum(acc);
        if (lane == 0) lg[cc] = acc + logit_b[cc];
    }
    __syncthreads();
}

// log-sum-exp of the logits and their maximum, C <= 64: one lane per category (v = the lane's logit, -inf where !in); whole wave
__device__ __forceinline__ float pos_lse_lanes(float v, bool in, float& mx) {
    mx = wave_max(v);
    return mx + logf(wave_sum(in ? expf(v - mx) : 0.f));
}

// the same for any C by one thread, in index order
__device__ __forceinline__ float pos_lse_serial(const float* lg, int C, float& mx) {
    mx = lg[0];
    for (int cc = 1; cc < C; ++cc) mx = fmaxf(mx, lg[cc]);
    float se = 0.f;
    for (int cc = 0; cc < C; ++cc) se += expf(lg[cc] - mx);
    return mx + logf(se);
}

// one workgroup per video: the cell (dropout is the identity in eval mode), then logit + log_softmax (SAModel.py:79-80 / :178)
// and, for greedy, the choice
__global__ void __launch_bounds__(STEP_TPB) pos_cell_head_kernel(CellHeadArgs a) {
    extern __shared__ float lds[];
    float* hs = lds;             // R
    float* lg = lds + a.R;       // C
    __shared__ float s_lse;
    const int b = blockIdx.x, tid = threadIdx.x, R = a.R, C = a.C, T = a.T, t = a.t;
    const bool tf = a.cap != nullptr;
    int64_t tk;
    float m;
    if (tf) {
        tk = a.cap[(size_t)b * T + t];
        m = a.new_mask[(size_t)b * T + t];
    } else {
        tk = t == 0 ? 0 : a.tok[b];
        m = t == 0 ? 1.0f : a.masks[(size_t)b * T + t];
    }
    tk = pos_clamp_tag(tk, C);
    const float* s = a.S + (size_t)b * 4 * R;
    const float* tb = a.tab + (size_t)tk * 4 * R;
    float* xh = a.X + (size_t)b * 2 * R + R;
    float* cb = a.c + (size_t)b * R;
    for (int j = tid; j < R; j += STEP_TPB) {
        const PosCell o = pos_cell(s, tb, R, j, cb[j], xh[j], m);
        cb[j] = o.cn;
        xh[j] = o.hn;
        hs[j] = o.hn;
        if (!tf) a.states[((size_t)b * T + t) * R + j] = o.hn;
    }
    if (!tf && t == 0 && tid == 0) a.masks[(size_t)b * T] = 1.0f;
    pos_head_logits(a.logit_w, a.logit_b, hs, lg, R, C);
    const int lane = tid & 63, wave = tid >> 6;
    const bool choose = !tf && t + 1 < T;
    float mx;
    if (C <= 64) {                                              // one lane per category
        if (wave == 0) {
            const float v = lane < C ? lg[lane] : -INFINITY;
            const float lse = pos_lse_lanes(v, lane < C, mx);
            if (lane == 0) s_lse = lse;
            if (choose) {
                const float lp = lane < C ? v - lse : -INFINITY;
                const float bv = wave_max(lp);
                const int best = __ffsll((unsigned long long)__ballot(lane < C && lp == bv)) - 1;
                if (lane == 0) pos_choose(a, b, best, bv);
            }
        }
    } else if (tid == 0) {
        const float lse = pos_lse_serial(lg, C, mx);
        s_lse = lse;
        if (choose) {
            int best = 0;
            float bv = lg[0] - lse;
            for (int cc = 1; cc < C; ++cc) {
                const float v = lg[cc] - lse;
                if (v > bv) { bv = v; best = cc; }
            }
            pos_choose(a, b, best, bv);
        }
    }
    if (tf) {
        __syncthreads();
        for (int cc = tid; cc < C; cc += STEP_TPB) a.logp[((size_t)b * T + t) * C + cc] = lg[cc] - s_lse;
    }
}

// out = the first column i >= 1 of the (B,T) matrix that is all zero, minus `sub` (T - sub when there is none): T' of the teacher-
// forced forward (int64 categories, sub 0) or n of the greedy rollout (float masks, sub 1)
__global__ void __launch_bounds__(POS_TPB) pos_first_zero_col_kernel(const int64_t* tokm, const float* maskm, int B, int T, int sub,
                                                                     int32_t* out) {
    int res = T - sub;
    for (int i = 1; i < T; ++i) {
        int nz = 0;
        for (int b = threadIdx.x; b < B; b += POS_TPB) nz |= tokm ? (tokm[(size_t)b * T + i] != 0) : (maskm[(size_t)b * T + i] != 0.0f);
        if (!__syncthreads_or(nz)) { res = i - sub; break; }
    }
    if (threadIdx.x == 0) out[0] = res;
}

const char* const kNames[] = {
    "two_fc_encoder.visual_emb_rgb.0.weight", "two_fc_encoder.visual_emb_rgb.0.bias",
    "two_fc_encoder.visual_emb_rgb.1.weight", "two_fc_encoder.visual_emb_rgb.1.bias",
    "two_fc_encoder.visual_emb_opfl.0.weight", "two_fc_encoder.visual_emb_opfl.0.bias",
    "two_fc_encoder.visual_emb_opfl.1.weight", "two_fc_encoder.visual_emb_opfl.1.bias",
    "two_fc_encoder.lstmcell_rgb.weight_ih", "two_fc_encoder.lstmcell_rgb.weight_hh",
    "two_fc_encoder.lstmcell_rgb.bias_ih", "two_fc_encoder.lstmcell_rgb.bias_hh",
    "two_fc_encoder.lstmcell_opfl.weight_ih", "two_fc_encoder.lstmcell_opfl.weight_hh",
    "two_fc_encoder.lstmcell_opfl.bias_ih", "two_fc_encoder.lstmcell_opfl.bias_hh",
    "two_fc_encoder.fusion.late_fusion.0.weight", "two_fc_encoder.fusion.late_fusion.0.bias",
    "img_embed_h_1.weight", "img_embed_h_1.bias", "img_embed_c_1.weight", "img_embed_c_1.bias",
    "lstmcore.lstmcell.i2h.weight", "lstmcore.lstmcell.i2h.bias", "lstmcore.lstmcell.a2h.weight", "lstmcore.lstmcell.a2h.bias",
    "lstmcore.lstmcell.h2h.weight", "lstmcore.lstmcell.h2h.bias",
    "lstmcore.v2a.weight", "lstmcore.v2a.bias", "lstmcore.h2a.weight", "lstmcore.h2a.bias", "lstmcore.a2w.weight", "lstmcore.a2w.bias",
    "embed.weight", "logit.weight", "logit.bias"};
constexpr int kNParams = (int)(sizeof(kNames) / sizeof(kNames[0]));
static_assert(kNParams * sizeof(float*) == sizeof(XgpParams), "one XgpParams field per name");

bool dims_ok(const XgpDims* d, bool need_t) {
    if (!d) return false;
    if (d->B <= 0 || d->K <= 0 || d->R <= 0 || d->A <= 0 || d->E <= 0 || d->C <= 0 || d->F1 <= 0 || d->F2 <= 0) return false;
    if (need_t && d->T <= 0) return false;
    // the workgroup-per-video kernels keep p, w (A each), the context parts and h (R) in LDS (under 64 KiB); 32-bit offsets
    if (d->A > 4096 || d->R > 4096 || d->C > 4096 || d->K > 1024) return false;
    return (int64_t)d->B * d->K * 4 * d->R < (1LL << 31) && (int64_t)d->B * (d->T > 0 ? d->T : 1) * d->R < (1LL << 31);
}

int64_t numel_of(const XgpDims* d, int i) {
    const int64_t R = d->R, A = d->A, E = d->E, C = d->C, F1 = d->F1, F2 = d->F2;
    switch (i) {
        case 0: return R * F1;
        case 4: return R * F2;
        case 1: case 2: case 3: case 5: case 6: case 7: return R;
        case 8: case 9: case 12: case 13: return 4 * R * R;
        case 10: case 11: case 14: case 15: return 4 * R;
        case 16: return R * 2 * R;
        case 17: return R;
        case 18: case 20: return R * R;
        case 19: case 21: return R;
        case 22: return 4 * R * E;
        case 24: case 26: return 4 * R * R;
        case 23: case 25: case 27: return 4 * R;
        case 28: case 30: return A * R;
        case 29: case 31: return A;
        case 32: return A;
        case 33: return 1;
        case 34: return C * E;
        case 35: return C * R;
        case 36: return C;
    }
    return -1;
}

// workspace regions in floats, each rounded up to 64 floats (256 bytes); every layout carves with one (base null: sizes only)
struct Carve {
    float* base;
    size_t off;
    float* take(size_t n) { float* r = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return r; }
    template <typename T> T* take(size_t n) { static_assert(sizeof(T) == sizeof(float), "counted in floats"); return (T*)take(n); }
};

struct Ws {
    float *Z, *Xe, *Pre, *S2, *c2, *hz, *Hcat, *V, *vbar, *Q, *tab, *X, *P, *S, *c;
    int64_t* tok;
    float *pk_h2a, *pk_a2h, *pk_h2h;   // the decoder step's weights packed for the fast skinny kernel
    size_t floats;
};

Ws ws_layout(const XgpDims* d, void* base) {
    const size_t B = d->B, K = d->K, R = d->R, A = d->A, C = d->C, BK = B * K;
    Carve cv{(float*)base, 0};
    Ws w;
    w.Z = cv.take(2 * BK * R);          // visual embeddings (rgb, opfl)
    w.Xe = cv.take(2 * BK * R);         // after BatchNorm + ReLU + frame mask
    w.Pre = cv.take(2 * BK * 4 * R);    // hoisted input side of the two encoder cells
    w.S2 = cv.take(2 * B * 4 * R);      // recurrent side of one frame
    w.c2 = cv.take(2 * B * R);
    w.hz = cv.take(B * R);              // zero state
    w.Hcat = cv.take(BK * 2 * R);       // [h_rgb ; h_opfl] of every frame
    w.V = cv.take(BK * R);
    w.vbar = cv.take(B * R);
    w.Q = cv.take(BK * A);              // v2a(V)
    w.tab = cv.take(C * 4 * R);         // embed i2h^T + i2h.bias
    w.X = cv.take(B * 2 * R);           // [af ; h]
    w.P = cv.take(B * A);
    w.S = cv.take(B * 4 * R);
    w.c = cv.take(B * R);
    w.tok = (int64_t*)cv.take(2 * B);
    w.pk_h2a = cv.take(packed_floats(A, R));
    w.pk_a2h = cv.take(packed_floats(4 * R, R));
    w.pk_h2h = cv.take(packed_floats(4 * R, R));
    w.floats = cv.off;
    return w;
}

// Y (M,N) = [A0 | A1] [W0 | W1]^T + bias (optionally ReLU'd): every product of the model, as ONE job of the captioner's skinny
// product launcher (xg_step.hip: xgk_skinny), over packed tiles (Bp0 / Bp1: the fast kernel) or the plain row-major weights (the
// LDS-staged kernel).  The job does not allow a cross-workgroup split (ksplit_ok = 0), so every output element has one fixed
// summation order and a call is bit-reproducible (xgk_gemm adds split-K partial tiles with atomics in arrival order on the
// skinny shapes of the decoder step).
int product(hipStream_t st, int M, int N, const float* A0, int lda0, const float* W0, int K0, const float* A1, int lda1,
            const float* W1, int K1, const float* bias, float* Y, int ldy, bool relu = false, const float* Bp0 = nullptr,
            const float* Bp1 = nullptr) {
    SkArgs a{};
    a.njobs = 1;
    SkJob& j = a.job[0];
    j.epi = SK_EPI_STORE;
    j.M = M; j.N = N; j.R = N;
    j.nseg = A1 ? 2 : 1;
    j.C = Y; j.ldc = ldy;
    j.relu = relu ? 1 : 0;
    const float* As[2] = {A0, A1};
    const float* Ws[2] = {W0, W1};
    const float* Bps[2] = {Bp0, Bp1};
    const int ld[2] = {lda0, lda1}, Ks[2] = {K0, K1};
    for (int q = 0; q < j.nseg; ++q) {
        SkSeg& sg = j.seg[q];
        sg.A = As[q]; sg.lda = ld[q]; sg.K = Ks[q]; sg.nck = xg_cdiv(Ks[q], 32);
        sg.B = Ws[q]; sg.ldb = Ks[q];
        sg.Bp = Bps[q];
    }
    j.bias[0] = bias;
    return xgk_skinny(st, a, 0);
}

bool params_ok(const XgpParams* p) {
    if (!p) return false;
    float* const* f = (float* const*)p;
    for (int i = 0; i < kNParams; ++i)
        if (!f[i]) return false;
    return true;
}

bool bn_ok(const XgBnState* bn) { return bn && bn->rgb_mean && bn->rgb_var && bn->opfl_mean && bn->opfl_var; }

constexpr float POS_BN_EPS = 1e-5f;

// one modality (rgb, opfl) of the encoder: its features and parameters out of XgpParams / XgBnState, then the recurrent loop's
// operands, set by the caller: the hoisted input side `pre` (B K,4R), the cell state before frame 0 `c0` (B,R), the states `cs`
// and, to keep them, the activated gates (B K,4R).  The parameter pointers are non-const on purpose: encoder_bwd fills a second
// pair from the gradient struct and adds into them (there only ew .. bhh mean anything); the forward encoders only read theirs.
struct EncMod {
    const float* feats;
    int F, site;
    float *ew, *eb, *bg, *bb, *rm, *rv, *wih, *whh, *bih, *bhh;
    const float *pre, *c0;
    float *cs, *gates;
};

void enc_mods(const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo, EncMod mo[2]) {
    mo[0] = EncMod{fr, d->F1, XG_SITE_EMB_RGB, p->emb_rgb_w, p->emb_rgb_b, p->bn_rgb_g, p->bn_rgb_b, bn ? bn->rgb_mean : nullptr,
                   bn ? bn->rgb_var : nullptr, p->lstm_rgb_wih, p->lstm_rgb_whh, p->lstm_rgb_bih, p->lstm_rgb_bhh};
    mo[1] = EncMod{fo, d->F2, XG_SITE_EMB_OPFL, p->emb_opfl_w, p->emb_opfl_b, p->bn_opfl_g, p->bn_opfl_b, bn ? bn->opfl_mean : nullptr,
                   bn ? bn->opfl_var : nullptr, p->lstm_opfl_wih, p->lstm_opfl_whh, p->lstm_opfl_bih, p->lstm_opfl_bhh};
}

// the two masked LSTM cells over the K frames into Hcat (B K,2R).  Frame k reads the cell state of frame k - 1 (c0 at k = 0) and
// writes cs + k cstep, row stride ldc: cstep 0 is one state in place, cstep R with ldc = K R keeps every frame's.  `hz`: zero h.
int encoder_recur(hipStream_t st, const XgpDims* d, const EncMod mo[2], const float* fm, const float* hz, float* S2, float* Hcat,
                  int cstep, int ldc, const XgDrop& drop) {
    const int B = d->B, K = d->K, R = d->R;
    for (int k = 0; k < K; ++k) {
        for (int m = 0; m < 2; ++m) {
            const float* hp = k == 0 ? hz : Hcat + (size_t)(k - 1) * 2 * R + m * R;
            float* S = S2 + (size_t)m * B * 4 * R;
            XG_TRY(product(st, B, 4 * R, hp, k == 0 ? R : K * 2 * R, mo[m].whh, R, nullptr, 0, nullptr, 0, mo[m].bhh, S, 4 * R));
            LstmFwdArgs a{};
            a.s = S; a.lds_ = 4 * R;
            a.add = mo[m].pre + (size_t)k * 4 * R; a.ldadd = K * 4 * R;
            a.c_prev = k == 0 ? mo[m].c0 : mo[m].cs + (size_t)(k - 1) * cstep; a.ldcp = k == 0 ? R : ldc;
            a.h_prev = nullptr; a.ldhp = 0;
            a.mask = fm + k; a.ldm = K;
            a.gates = mo[m].gates ? mo[m].gates + (size_t)k * 4 * R : nullptr; a.ldg = mo[m].gates ? K * 4 * R : 0;
            a.c_out = mo[m].cs + (size_t)k * cstep; a.ldco = ldc;
            a.h_out = Hcat + (size_t)k * 2 * R + m * R; a.ldho = K * 2 * R;
            a.B = B; a.R = R; a.order = XG_ORDER_IFGO; a.mask_mode = XG_MASK_ZERO;
            a.drop = drop;
            XG_TRY(xgk_lstm_fwd(st, a));
        }
    }
    return XG_OK;
}

// eval-mode encoder (pos_src/sub_modules.py:199-239) into V (B*K rows of R)
int encoder(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo,
            const float* fm, float* V, const Ws& w) {
    const int B = d->B, K = d->K, R = d->R, BK = B * K;
    const size_t BKR = (size_t)BK * R;
    XgDrop nodrop;
    nodrop.seed = 0; nodrop.site = 0; nodrop.step = 0; nodrop.thresh = 0u; nodrop.scale = 1.0f;
    EncMod mo[2];
    enc_mods(d, p, bn, fr, fo, mo);
    for (int m = 0; m < 2; ++m) {
        EncMod& e = mo[m];
        float* Z = w.Z + m * BKR;
        float* Xe = w.Xe + m * BKR;
        float* Pre = w.Pre + m * BKR * 4;
        XG_TRY(product(st, BK, R, e.feats, e.F, e.ew, e.F, nullptr, 0, nullptr, 0, e.eb, Z, R));
        // eval BatchNorm with the running statistics, ReLU, then the frame mask (the dropout is the identity)
        XG_TRY(xgk_bn_apply(st, Z, e.rm, e.rv, e.bg, e.bb, fm, Xe, BK, R, POS_BN_EPS, nodrop));
        XG_TRY(product(st, BK, 4 * R, Xe, R, e.wih, R, nullptr, 0, nullptr, 0, e.bih, Pre, 4 * R));
        e.pre = Pre;
        e.c0 = e.cs = w.c2 + (size_t)m * B * R;     // one state per modality, zeroed here and updated in place
        XG_TRY(xgk_fill(st, e.cs, 0.f, (int64_t)B * R));
    }
    XG_TRY(xgk_fill(st, w.hz, 0.f, (int64_t)B * R));
    XG_TRY(encoder_recur(st, d, mo, fm, w.hz, w.S2, w.Hcat, 0, R, nodrop));
    // late fusion: relu(W [h_rgb ; h_opfl] + b); masked frames carry relu(b)
    return product(st, BK, R, w.Hcat, 2 * R, p->fusion_w, 2 * R, nullptr, 0, nullptr, 0, p->fusion_b, V, R, true);
}

// the per-call hoisted operands of the decoder step, eval and train alike: Q = v2a(V), the token table tab = embed i2h^T with the
// three biases folded in, and the step's weights packed for the fast skinny kernel
int hoist_operands(hipStream_t st, const XgpDims* d, const XgpParams* p, const float* V, float* Q, float* tab, float* pk_h2a,
                   float* pk_a2h, float* pk_h2h) {
    const int B = d->B, K = d->K, R = d->R, A = d->A, E = d->E, C = d->C;
    XG_TRY(product(st, B * K, A, V, R, p->v2a_w, R, nullptr, 0, nullptr, 0, p->v2a_b, Q, A));
    XG_TRY(product(st, C, 4 * R, p->embed_w, E, p->i2h_w, E, nullptr, 0, nullptr, 0, p->i2h_b, tab, 4 * R));
    hipLaunchKernelGGL(pos_pack_kernel, dim3(xg_cdiv(A, 32) * xg_cdiv(R, 32)), dim3(POS_TPB), 0, st, p->h2a_w, A, R, pk_h2a);
    hipLaunchKernelGGL(pos_pack_kernel, dim3(xg_cdiv(4 * R, 32) * xg_cdiv(R, 32)), dim3(POS_TPB), 0, st, p->a2h_w, 4 * R, R, pk_a2h);
    hipLaunchKernelGGL(pos_pack_kernel, dim3(xg_cdiv(4 * R, 32) * xg_cdiv(R, 32)), dim3(POS_TPB), 0, st, p->h2h_w, 4 * R, R, pk_h2h);
    XG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pos_fold_bias_kernel, dim3(xg_cdiv(C * 4 * R, POS_TPB)), dim3(POS_TPB), 0, st, tab, p->a2h_b, p->h2h_b, C, 4 * R);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// encoder, init_hidden (SAModel.py:54-60: the sum of V over all K rows over the mask count) into X[:, R:2R] and c, and the hoisted
// operands
int prologue(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo,
             const float* fm, const Ws& w) {
    const int B = d->B, K = d->K, R = d->R;
    XG_TRY(encoder(st, d, p, bn, fr, fo, fm, w.V, w));
    XG_TRY(xgk_masked_mean(st, w.V, fm, w.vbar, B, K, R));
    XG_TRY(product(st, B, R, w.vbar, R, p->ih1_w, R, nullptr, 0, nullptr, 0, p->ih1_b, w.X + R, 2 * R));
    XG_TRY(product(st, B, R, w.vbar, R, p->ic1_w, R, nullptr, 0, nullptr, 0, p->ic1_b, w.c, R));
    return hoist_operands(st, d, p, w.V, w.Q, w.tab, w.pk_h2a, w.pk_a2h, w.pk_h2h);
}

// step_front: the first three launches of the decoder step, the same in every eval call, over M = B S rows (row b S + s) with the
// operands X (M,2R), P (M,A), S (M,4R) and the videos' hoisted operands `v`.  The plan is what the attention launch needs beyond
// that, computed once per call before the time loop.  (Both are defined below pos_attn_group_kernel, the attention of S > 1.)
struct StepPlan {
    int S;                       // rows per video
    int G;                       // 0: pos_attn_kernel (S = 1), else pos_attn_group_kernel<G>
    int nsplit, pr_floats;
    size_t lds;                  // the attention's dynamic LDS bytes
    bool v4;
};
StepPlan step_plan(const XgpDims* d, int S);
// pos_attn_kernel over B rows, each with its own video (the plan's S = 1 form)
void launch_attn(hipStream_t st, int B, const StepPlan& pl, const float* P, const float* Q, const float* V, const float* w, float* X,
                 int K, int R, int A) {
    if (pl.v4) hipLaunchKernelGGL(pos_attn_kernel<true>, dim3(B), dim3(STEP_TPB), pl.lds, st, P, Q, V, w, X, K, R, A, pl.nsplit);
    else       hipLaunchKernelGGL(pos_attn_kernel<false>, dim3(B), dim3(STEP_TPB), pl.lds, st, P, Q, V, w, X, K, R, A, pl.nsplit);
}

int step_front(hipStream_t st, const XgpDims* d, const XgpParams* p, const StepPlan& pl, const Ws& v, float* X, float* P, float* S);

// the prologue, the T decoder steps, then the early exit into `out`.  ca.cap set is the teacher-forced call (T' from the categories,
// sub 0), null the greedy one (n from ca.masks, sub 1): the same test pos_cell_head_kernel makes (`tf`)
int decode(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo, const float* fm,
           CellHeadArgs ca, int32_t* out, const Ws& w) {
    const int B = d->B, R = d->R, C = d->C, T = d->T;
    XG_TRY(prologue(st, d, p, bn, fr, fo, fm, w));
    ca.S = w.S; ca.tab = w.tab; ca.logit_w = p->logit_w; ca.logit_b = p->logit_b;
    ca.X = w.X; ca.c = w.c; ca.B = B; ca.R = R; ca.C = C; ca.T = T;
    const StepPlan pl = step_plan(d, 1);
    for (int t = 0; t < T; ++t) {
        XG_TRY(step_front(st, d, p, pl, w, w.X, w.P, w.S));
        ca.t = t;
        hipLaunchKernelGGL(pos_cell_head_kernel, dim3(B), dim3(STEP_TPB), (size_t)(R + C) * sizeof(float), st, ca);
        XG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pos_first_zero_col_kernel, dim3(1), dim3(POS_TPB), 0, st, ca.cap, ca.masks, B, T, ca.cap ? 0 : 1, out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// the argument gate of every entry point, after the test of its own dims, scalars and pointers: parameters, running statistics
// (bn_good: true for a call that takes none), features, ws, then its size against the call's layout (`floats`).  XG_EINVAL first.
int args_gate(const XgpParams* p, bool bn_good, const float* fr, const float* fo, const float* fm, void* ws, size_t ws_bytes,
              size_t floats) {
    if (!params_ok(p) || !bn_good || !fr || !fo || !fm || !ws) return XG_EINVAL;
    return ws_bytes < floats * sizeof(float) ? XG_EWORKSPACE : XG_OK;
}

int common_checks(const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo, const float* fm,
                  void* ws, size_t ws_bytes, bool need_t) {
    if (!dims_ok(d, need_t)) return XG_EINVAL;
    return args_gate(p, bn_ok(bn), fr, fo, fm, ws, ws_bytes, ws_layout(d, nullptr).floats);
}

}  // namespace

extern "C" int xgp_version(void) { return XGP_VERSION; }
extern "C" int xgp_param_count(void) { return kNParams; }
extern "C" const char* xgp_param_name(int i) { return i >= 0 && i < kNParams ? kNames[i] : nullptr; }

extern "C" int xgp_param_numel(const XgpDims* d, int i, int64_t* numel) {
    if (!dims_ok(d, false) || i < 0 || i >= kNParams || !numel) return XG_EINVAL;
    *numel = numel_of(d, i);
    return XG_OK;
}

extern "C" size_t xgp_workspace_bytes(const XgpDims* d) {
    if (!dims_ok(d, false)) return 0;
    return ws_layout(d, nullptr).floats * sizeof(float);
}

extern "C" int xgp_encoder_fwd(void* stream, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* feats_rgb,
                               const float* feats_opfl, const float* feat_mask, float* V, void* ws, size_t ws_bytes) {
    XG_TRY(common_checks(d, p, bn, feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, false));
    if (!V) return XG_EINVAL;
    return encoder((hipStream_t)stream, d, p, bn, feats_rgb, feats_opfl, feat_mask, V, ws_layout(d, ws));
}

extern "C" int xgp_forward_tf(void* stream, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* feats_rgb,
                              const float* feats_opfl, const float* feat_mask, const int64_t* cap_classes, const float* new_mask,
                              float* logp, int32_t* t_out, void* ws, size_t ws_bytes) {
    XG_TRY(common_checks(d, p, bn, feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, true));
    if (!cap_classes || !new_mask || !logp || !t_out) return XG_EINVAL;
    CellHeadArgs ca{};
    ca.cap = cap_classes; ca.new_mask = new_mask; ca.logp = logp;
    return decode((hipStream_t)stream, d, p, bn, feats_rgb, feats_opfl, feat_mask, ca, t_out, ws_layout(d, ws));
}

extern "C" int xgp_sample_greedy(void* stream, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const float* feats_rgb,
                                 const float* feats_opfl, const float* feat_mask, int64_t* seq, float* seq_logp, float* states,
                                 float* masks, int32_t* n_out, void* ws, size_t ws_bytes) {
    XG_TRY(common_checks(d, p, bn, feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, true));
    if (d->T < 2 || !seq || !seq_logp || !states || !masks || !n_out) return XG_EINVAL;
    const Ws w = ws_layout(d, ws);
    CellHeadArgs ca{};
    ca.tok = w.tok; ca.masks = masks; ca.seq = seq; ca.seq_logp = seq_logp; ca.states = states;
    return decode((hipStream_t)stream, d, p, bn, feats_rgb, feats_opfl, feat_mask, ca, n_out, w);
}

// ==================================================================================================================================
// Training (include/xgate_pos_train.h): the teacher-forced iteration of pos_src/starttrain_trainpos.py:138-152.
//
// Forward, train mode: the eval forward's launch structure with BatchNorm over the batch statistics (running statistics updated in
// the same launch), hash dropout at sites 0 / 1 (embeddings), 4 (fusion) and 6 (decoder cell, step t), and every activation the
// backward needs kept in the workspace: per step p = h2a(h), alpha, af, the activated gates, h and c (before and after) and the
// log-probabilities.  The attention of a step is the captioner's xgk_attn_fwd (it keeps alpha); the cell epilogue and the head are
// pos_cell_head_train_kernel.
// Backward, per step in reverse: pos_cell_head_bwd_kernel (log_softmax backward, dlogits logit_w into dh, then the cell backward with
// the HOLD mask and the site-6 dropout), daf = ds a2h_w, xgk_attn_bwd, and dh_prev += ds h2h_w + dp h2a_w as one two-segment
// skinny job.  After the loop every weight gradient is one batched product over the T' B rows; then the encoder in reverse.
// ==================================================================================================================================
#include "../../include/xgate_pos_train.h"
#include "../../include/xgate_pos_joint.h"

namespace {

XgDrop pos_drop(const XgptRun* run, uint32_t site, uint32_t step) {
    XgDrop d;
    d.seed = run->seed; d.site = site; d.step = step;
    if (run->train && run->drop_p > 0.f) {
        const double t = (double)run->drop_p * 4294967296.0;
        d.thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
        d.scale = 1.0f / (1.0f - run->drop_p);
    } else {
        d.thresh = 0u;
        d.scale = 1.0f;
    }
    return d;
}

// pos_pack_kernel for a (K,N) row-major source: the tiles of its transpose, i.e. the B operand of Y = A W for the backward's
// data-gradient products dX = dY W
__global__ void __launch_bounds__(POS_TPB) pos_pack_t_kernel(const float* __restrict__ src, int N, int K, float* __restrict__ dst) {
    __shared__ float t[32][33];
    const int nck = (K + 31) >> 5;
    const int tile = blockIdx.x, tn = tile / nck, kc = tile - tn * nck;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kk = ty + 8 * r, k = kc * 32 + kk, n = tn * 32 + tx;
        t[tx][kk] = (n < N && k < K) ? src[(size_t)k * N + n] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = threadIdx.x + POS_TPB * r;
        const int q = o & 3, nn = (o >> 2) & 31, h = (o >> 7) & 1, i = o >> 8;
        dst[(size_t)tile * 1024 + o] = t[nn][16 * h + 4 * i + q];
    }
}

struct CellTrainArgs {
    const float* S;              // (B,4R) af a2h^T + h h2h^T, no bias
    const float* tab;            // (C,4R) embed i2h^T + the three biases
    const float *logit_w, *logit_b;
    const int64_t* cap; const float* new_mask;     // (B,T)
    const float *h_prev, *c_prev;                   // (B,R) state before the step
    float *h_out, *c_out;                           // (B,R) state after the step (h: after the dropout)
    float* gates;                                   // (B,4R) activated gates, order i,f,o,g
    float* lp;                                      // (B,C) log-probabilities of the step (saved)
    float* logp;                                    // (B,T,C) output
    int B, R, C, T, t;
    XgDrop drop;
};

// one workgroup per video: pos_cell_head_kernel's teacher-forced path plus the dropout of h after the mask hold
// (sub_modules.py:884-887: the dropped h is the state AND the head's input) and the saved gates
__global__ void __launch_bounds__(STEP_TPB) pos_cell_head_train_kernel(CellTrainArgs a) {
    extern __shared__ float lds[];
    float* hs = lds;             // R
    float* lg = lds + a.R;       // C
    __shared__ float s_lse;
    const int b = blockIdx.x, tid = threadIdx.x, R = a.R, C = a.C, T = a.T, t = a.t;
    const int64_t tk = pos_clamp_tag(a.cap[(size_t)b * T + t], C);
    const float m = a.new_mask[(size_t)b * T + t];
    const float* s = a.S + (size_t)b * 4 * R;
    const float* tb = a.tab + (size_t)tk * 4 * R;
    float* gb = a.gates + (size_t)b * 4 * R;
    for (int j = tid; j < R; j += STEP_TPB) {
        const PosCell o = pos_cell(s, tb, R, j, a.c_prev[(size_t)b * R + j], a.h_prev[(size_t)b * R + j], m);
        const float hn = o.hn * xg_keep(a.drop, (uint32_t)(b * R + j));
        gb[j] = o.ig; gb[R + j] = o.fg; gb[2 * R + j] = o.og; gb[3 * R + j] = o.gg;
        a.c_out[(size_t)b * R + j] = o.cn;
        a.h_out[(size_t)b * R + j] = hn;
        hs[j] = hn;
    }
    pos_head_logits(a.logit_w, a.logit_b, hs, lg, R, C);
    const int lane = tid & 63, wave = tid >> 6;
    // (chunks of 64 rather than pos_lse_lanes / pos_lse_serial: for C > 64 the wave sums in another order than the serial form)
    if (wave == 0) {
        float mx = -INFINITY;
        for (int c0 = 0; c0 < C; c0 += 64) mx = fmaxf(mx, wave_max(c0 + lane < C ? lg[c0 + lane] : -INFINITY));
        float se = 0.f;
        for (int c0 = 0; c0 < C; c0 += 64) se += wave_sum(c0 + lane < C ? expf(lg[c0 + lane] - mx) : 0.f);
        if (lane == 0) s_lse = mx + logf(se);
    }
    __syncthreads();
    for (int cc = tid; cc < C; cc += STEP_TPB) {
        const float v = lg[cc] - s_lse;
        a.lp[(size_t)b * C + cc] = v;
        a.logp[((size_t)b * T + t) * C + cc] = v;
    }
}

struct CellBwdArgs {
    const float* lp;             // (B,C) saved log-probabilities of the step
    const float* dlogp;          // (B,Tp,C) incoming gradient; null: all zero (nothing is read)
    const float* logit_w;        // (C,R)
    const float* gates;          // (B,4R) i,f,o,g
    const float *c_prev, *c_out; // (B,R)
    const float* new_mask;       // (B,T)
    const float* dh_in;          // (B,R) dh of the step's output from the later steps
    float* dh_out;               // (B,R) overwritten with (1 - m) du: the products of the step then add into it
    float* dc;                   // (B,R) in: dc of the step's cell state, out: dc of the previous one
    float* ds;                   // (B,4R)
    float* dlogits;              // (B,C)
    int B, R, C, T, Tp, t;
    XgDrop drop;
};

// one workgroup per video, the mirror of pos_cell_head_train_kernel: dlogits = dlogp - exp(lp) sum(dlogp), dh = dlogits logit_w +
// the carried dh, then the two_inputs_lstmcell backward (HOLD mask, dropout after the hold)
__global__ void __launch_bounds__(STEP_TPB) pos_cell_head_bwd_kernel(CellBwdArgs a) {
    extern __shared__ float lds[];
    float* dl = lds;             // C
    const int b = blockIdx.x, tid = threadIdx.x, R = a.R, C = a.C, t = a.t;
    const int lane = tid & 63, wave = tid >> 6;
    const float* lpb = a.lp + (size_t)b * C;
    const float* dlp = a.dlogp ? a.dlogp + ((size_t)b * a.Tp + t) * C : nullptr;
    if (wave == 0 && !dlp) {                     // no gradient for the log-probabilities: dlogits = 0, the head sends nothing
        for (int cc = lane; cc < C; cc += 64) {
            dl[cc] = 0.f;
            a.dlogits[(size_t)b * C + cc] = 0.f;
        }
    } else if (wave == 0) {
        float sd = 0.f;
        for (int c0 = 0; c0 < C; c0 += 64) sd += wave_sum(c0 + lane < C ? dlp[c0 + lane] : 0.f);
        for (int cc = lane; cc < C; cc += 64) {
            const float v = dlp[cc] - __expf(lpb[cc]) * sd;
            dl[cc] = v;
            a.dlogits[(size_t)b * C + cc] = v;
        }
    }
    __syncthreads();
    const float m = a.new_mask[(size_t)b * a.T + t];
    const float* g = a.gates + (size_t)b * 4 * R;
    float* ds = a.ds + (size_t)b * 4 * R;
    for (int j = tid; j < R; j += STEP_TPB) {
        float head = 0.f;
        for (int cc = 0; cc < C; ++cc) head += dl[cc] * a.logit_w[(size_t)cc * R + j];
        const size_t e = (size_t)b * R + j;
        const float du = (a.dh_in[e] + head) * xg_keep(a.drop, (uint32_t)e);
        const float ig = g[j], fg = g[R + j], og = g[2 * R + j], gg = g[3 * R + j];
        const float cp = a.c_prev[e], tc = xg_tanh(a.c_out[e]);
        const float dht = m * du;
        const float dcs = a.dc[e] + dht * og * (1.0f - tc * tc);
        const float dct = m * dcs;
        a.dh_out[e] = (1.0f - m) * du;
        a.dc[e] = (1.0f - m) * dcs + dct * fg;
        ds[j] = dct * gg * ig * (1.0f - ig);
        ds[R + j] = dct * cp * fg * (1.0f - fg);
        ds[2 * R + j] = dht * tc * og * (1.0f - og);
        ds[3 * R + j] = dct * ig * (1.0f - gg * gg);
    }
}

// Hprev (B,K,R): row (b, k) = h of frame k - 1 of modality m (zero at k = 0), from Hcat (B,K,2R)
__global__ void __launch_bounds__(POS_TPB) pos_shift_h_kernel(const float* __restrict__ Hcat, int m, int K, int R, int64_t n,
                                                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * POS_TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / R;
    const int r = (int)(i - row * R), k = (int)(row % K);
    out[i] = k == 0 ? 0.f : Hcat[(row - 1) * 2 * R + (size_t)m * R + r];
}

struct TWs {
    // forward (saved)
    float *Z[2], *Xe[2], *mean[2], *var[2], *Pre[2], *G[2], *Cs[2];
    float *S2, *zero, *Hcat, *V, *vbar, *Q, *tab;
    float *Hst, *Cst, *P, *ALPHA, *AF, *GD, *LP, *S, *nm;
    int64_t* cap;
    float *pk_h2a, *pk_a2h, *pk_h2h, *pkt_a2h, *pkt_h2h, *pkt_h2a;
    // backward
    float *dH[2], *dC, *DS, *DP, *DAF, *DE, *DLOG, *Xemb, *DXemb, *DVPROJ, *DV, *dVw, *dHcat, *dHrec[2], *dCrec[2][2], *dS[2],
        *Hprev, *dX, *bn_s1, *bn_s2;
    size_t floats;
};

TWs tws_layout(const XgpDims* d, void* base) {
    const size_t B = d->B, K = d->K, R = d->R, A = d->A, C = d->C, E = d->E, T = d->T, BK = B * K;
    Carve cv{(float*)base, 0};
    TWs w;
    for (int m = 0; m < 2; ++m) {
        w.Z[m] = cv.take(BK * R); w.Xe[m] = cv.take(BK * R); w.mean[m] = cv.take(R); w.var[m] = cv.take(R);
        w.Pre[m] = cv.take(BK * 4 * R); w.G[m] = cv.take(BK * 4 * R); w.Cs[m] = cv.take(BK * R);
    }
    w.S2 = cv.take(2 * B * 4 * R); w.zero = cv.take(B * R); w.Hcat = cv.take(BK * 2 * R); w.V = cv.take(BK * R); w.vbar = cv.take(B * R);
    w.Q = cv.take(BK * A); w.tab = cv.take(C * 4 * R);
    w.Hst = cv.take((T + 1) * B * R); w.Cst = cv.take((T + 1) * B * R); w.P = cv.take(T * B * A); w.ALPHA = cv.take(T * B * K);
    w.AF = cv.take(T * B * R); w.GD = cv.take(T * B * 4 * R); w.LP = cv.take(T * B * C); w.S = cv.take(B * 4 * R); w.nm = cv.take(B * T);
    w.cap = (int64_t*)cv.take(2 * B * T);
    w.pk_h2a = cv.take(packed_floats(A, R)); w.pk_a2h = cv.take(packed_floats(4 * R, R)); w.pk_h2h = cv.take(packed_floats(4 * R, R));
    w.pkt_a2h = cv.take(packed_floats(R, 4 * R)); w.pkt_h2h = cv.take(packed_floats(R, 4 * R)); w.pkt_h2a = cv.take(packed_floats(R, A));
    w.dH[0] = cv.take(B * R); w.dH[1] = cv.take(B * R); w.dC = cv.take(B * R);
    w.DS = cv.take(T * B * 4 * R); w.DP = cv.take(T * B * A); w.DAF = cv.take(T * B * R); w.DE = cv.take(T * B * K); w.DLOG = cv.take(T * B * C);
    w.Xemb = cv.take(T * B * E); w.DXemb = cv.take(T * B * E); w.DVPROJ = cv.take(BK * A); w.DV = cv.take(BK * R); w.dVw = cv.take(BK * R);
    w.dHcat = cv.take(BK * 2 * R);
    for (int m = 0; m < 2; ++m) {
        w.dHrec[m] = cv.take(B * R); w.dCrec[m][0] = cv.take(B * R); w.dCrec[m][1] = cv.take(B * R); w.dS[m] = cv.take(BK * 4 * R);
    }
    w.Hprev = cv.take(BK * R); w.dX = cv.take(BK * R); w.bn_s1 = cv.take(R); w.bn_s2 = cv.take(R);
    w.floats = cv.off;
    return w;
}

// Y (M,N) (+)= A0 W0 (+ A1 W1) with W_q (K_q, N) row-major: the data-gradient products of the backward as ONE skinny job (packed
// transposed tiles Bp_q: the fast kernel; none: the LDS-staged kernel)
int product_nn(hipStream_t st, int M, int N, float* Y, int ldy, bool acc, const float* A0, int lda0, const float* W0, int K0,
               const float* Bp0, const float* A1 = nullptr, int lda1 = 0, const float* W1 = nullptr, int K1 = 0,
               const float* Bp1 = nullptr) {
    SkArgs a{};
    a.njobs = 1;
    SkJob& j = a.job[0];
    j.epi = SK_EPI_STORE;
    j.M = M; j.N = N; j.R = N;
    j.nseg = A1 ? 2 : 1;
    j.C = Y; j.ldc = ldy;
    j.accumulate = acc ? 1 : 0;
    const float* As[2] = {A0, A1};
    const float* Ws[2] = {W0, W1};
    const float* Bps[2] = {Bp0, Bp1};
    const int ld[2] = {lda0, lda1}, Ks[2] = {K0, K1};
    for (int q = 0; q < j.nseg; ++q) {
        SkSeg& sg = j.seg[q];
        sg.A = As[q]; sg.lda = ld[q]; sg.K = Ks[q]; sg.nck = xg_cdiv(Ks[q], 32);
        sg.B = Ws[q]; sg.ldb = N; sg.b_ncontig = 1;
        sg.Bp = Bps[q];
    }
    return xgk_skinny(st, a, 0);
}

// dW (N,K) += dY (M,N)^T X (M,K) and the bias gradient(s) of dY
int wgrad(hipStream_t st, int M, int N, int K, const float* dY, int lddy, const float* X, int ldx, float* dW, float* b1,
          float* b2 = nullptr, float* b3 = nullptr) {
    return xgk_gemm_cs(st, 0, true, false, N, K, M, dY, lddy, X, ldx, dW, K, nullptr, false, true, b1, b2, b3);
}
// dX (M,N) (+)= dY (M,K) W (K,N)
int dgrad(hipStream_t st, int M, int N, int K, const float* dY, int lddy, const float* W, float* dX, int lddx, bool acc) {
    return xgk_gemm(st, 0, false, false, M, N, K, dY, lddy, W, N, dX, lddx, nullptr, false, acc);
}

void pack_t(hipStream_t st, const float* W, int N, int K, float* dst) {
    hipLaunchKernelGGL(pos_pack_t_kernel, dim3(xg_cdiv(N, 32) * xg_cdiv(K, 32)), dim3(POS_TPB), 0, st, W, N, K, dst);
}

int encoder_train(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const XgptRun* run, const float* fr,
                  const float* fo, const float* fm, const TWs& w) {
    const int B = d->B, K = d->K, R = d->R, BK = B * K;
    EncMod mo[2];
    enc_mods(d, p, bn, fr, fo, mo);
    XgptRun nd = *run;
    nd.drop_p = 0.f;
    for (int m = 0; m < 2; ++m) {
        EncMod& e = mo[m];
        XG_TRY(product(st, BK, R, e.feats, e.F, e.ew, e.F, nullptr, 0, nullptr, 0, e.eb, w.Z[m], R));
        const XgDrop drop = pos_drop(run, e.site, 0);
        if (run->train) {
            // batch statistics over all B K rows (masked frames included, as nn.BatchNorm1d sees them) + the running update
            const int rc = xgk_bn_train_fwd(st, w.Z[m], BK, R, w.mean[m], w.var[m], e.rm, e.rv, run->bn_momentum, e.bg, e.bb, fm,
                                            w.Xe[m], POS_BN_EPS, drop);
            if (rc == 1) {
                XG_TRY(xgk_bn_stats(st, w.Z[m], BK, R, w.mean[m], w.var[m], e.rm, e.rv, run->bn_momentum));
                XG_TRY(xgk_bn_apply(st, w.Z[m], w.mean[m], w.var[m], e.bg, e.bb, fm, w.Xe[m], BK, R, POS_BN_EPS, drop));
            } else if (rc != XG_OK) {
                return rc;
            }
        } else {
            if (hipMemcpyAsync(w.mean[m], e.rm, sizeof(float) * R, hipMemcpyDeviceToDevice, st) != hipSuccess) return XG_EHIP;
            if (hipMemcpyAsync(w.var[m], e.rv, sizeof(float) * R, hipMemcpyDeviceToDevice, st) != hipSuccess) return XG_EHIP;
            XG_TRY(xgk_bn_apply(st, w.Z[m], w.mean[m], w.var[m], e.bg, e.bb, fm, w.Xe[m], BK, R, POS_BN_EPS, drop));
        }
        XG_TRY(product(st, BK, 4 * R, w.Xe[m], R, e.wih, R, nullptr, 0, nullptr, 0, e.bih, w.Pre[m], 4 * R));
        e.pre = w.Pre[m]; e.c0 = w.zero; e.cs = w.Cs[m]; e.gates = w.G[m];     // the backward reads every frame's state and gates
    }
    XG_TRY(xgk_fill(st, w.zero, 0.f, (int64_t)B * R));
    XG_TRY(encoder_recur(st, d, mo, fm, w.zero, w.S2, w.Hcat, R, K * R, pos_drop(&nd, 0, 0)));
    // late fusion: dropout(relu(W [h_rgb ; h_opfl] + b)) (sub_modules.py:63-66)
    XG_TRY(product(st, BK, R, w.Hcat, 2 * R, p->fusion_w, 2 * R, nullptr, 0, nullptr, 0, p->fusion_b, w.V, R, true));
    return xgk_relu_drop_fwd(st, w.V, (int64_t)BK * R, pos_drop(run, XG_SITE_FUSION, 0));
}

int forward_train(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const XgptRun* run, const float* fr,
                  const float* fo, const float* fm, const int64_t* cap, const float* nm, float* logp, const TWs& w) {
    const int B = d->B, K = d->K, R = d->R, A = d->A, C = d->C, T = d->T;
    const size_t BR = (size_t)B * R;
    if (hipMemcpyAsync(w.cap, cap, sizeof(int64_t) * B * T, hipMemcpyDeviceToDevice, st) != hipSuccess) return XG_EHIP;
    if (hipMemcpyAsync(w.nm, nm, sizeof(float) * B * T, hipMemcpyDeviceToDevice, st) != hipSuccess) return XG_EHIP;
    XG_TRY(encoder_train(st, d, p, bn, run, fr, fo, fm, w));
    XG_TRY(xgk_masked_mean(st, w.V, fm, w.vbar, B, K, R));                 // (detached: SAModel.py:54-60)
    XG_TRY(product(st, B, R, w.vbar, R, p->ih1_w, R, nullptr, 0, nullptr, 0, p->ih1_b, w.Hst, R));
    XG_TRY(product(st, B, R, w.vbar, R, p->ic1_w, R, nullptr, 0, nullptr, 0, p->ic1_b, w.Cst, R));
    XG_TRY(hoist_operands(st, d, p, w.V, w.Q, w.tab, w.pk_h2a, w.pk_a2h, w.pk_h2h));
    CellTrainArgs ca{};
    ca.S = w.S; ca.tab = w.tab; ca.logit_w = p->logit_w; ca.logit_b = p->logit_b;
    ca.cap = w.cap; ca.new_mask = w.nm; ca.logp = logp;
    ca.B = B; ca.R = R; ca.C = C; ca.T = T;
    const size_t lds_cell = (size_t)(R + C) * sizeof(float);
    for (int t = 0; t < T; ++t) {
        const float* h = w.Hst + t * BR;
        float* P = w.P + (size_t)t * B * A;
        float* af = w.AF + t * BR;
        XG_TRY(product(st, B, A, h, R, p->h2a_w, R, nullptr, 0, nullptr, 0, p->h2a_b, P, A, false, w.pk_h2a));
        XG_TRY(xgk_attn_fwd(st, P, w.Q, w.V, p->a2w_w, w.ALPHA + (size_t)t * B * K, af, B, K, R, A));
        XG_TRY(product(st, B, 4 * R, af, R, p->a2h_w, R, h, R, p->h2h_w, R, nullptr, w.S, 4 * R, false, w.pk_a2h, w.pk_h2h));
        ca.t = t;
        ca.h_prev = h; ca.c_prev = w.Cst + t * BR;
        ca.h_out = w.Hst + (t + 1) * BR; ca.c_out = w.Cst + (t + 1) * BR;
        ca.gates = w.GD + (size_t)t * B * 4 * R;
        ca.lp = w.LP + (size_t)t * B * C;
        ca.drop = pos_drop(run, XG_SITE_L1, (uint32_t)t);
        hipLaunchKernelGGL(pos_cell_head_train_kernel, dim3(B), dim3(STEP_TPB), lds_cell, st, ca);
        XG_CHECK_LAUNCH();
    }
    return XG_OK;
}

int encoder_bwd(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgpParams* g, const XgptRun* run, const float* fr,
                const float* fo, const float* fm, const TWs& w) {
    const int B = d->B, K = d->K, R = d->R, BK = B * K;
    EncMod mo[2], gm[2];         // the parameters, and where their gradients go
    enc_mods(d, p, nullptr, fr, fo, mo);
    enc_mods(d, g, nullptr, nullptr, nullptr, gm);
    XgptRun nd = *run;
    nd.drop_p = 0.f;
    // fusion: dVw = dV keep (V > 0), then its weight gradient and dHcat
    XG_TRY(xgk_relu_drop_bwd(st, w.dVw, w.V, (int64_t)BK * R, pos_drop(run, XG_SITE_FUSION, 0), w.DV));
    XG_TRY(wgrad(st, BK, R, 2 * R, w.dVw, R, w.Hcat, 2 * R, g->fusion_w, g->fusion_b));
    XG_TRY(dgrad(st, BK, 2 * R, R, w.dVw, R, p->fusion_w, w.dHcat, 2 * R, false));
    for (int m = 0; m < 2; ++m) {
        XG_TRY(xgk_fill(st, w.dHrec[m], 0.f, (int64_t)B * R));
        XG_TRY(xgk_fill(st, w.dCrec[m][0], 0.f, (int64_t)B * R));
    }
    int c = 0;
    auto cell = [&](int m, int i) {
        LstmBwdArgs a{};
        a.gates = w.G[m] + (size_t)i * 4 * R; a.ldg = K * 4 * R;
        a.c_prev = i == 0 ? w.zero : w.Cs[m] + (size_t)(i - 1) * R; a.ldcp = i == 0 ? R : K * R;
        a.c_out = w.Cs[m] + (size_t)i * R; a.ldco = K * R;
        a.mask = fm + i; a.ldm = K;
        a.dh_out = w.dHcat + (size_t)i * 2 * R + m * R; a.lddh = K * 2 * R;
        a.dh_add = w.dHrec[m]; a.lddha = R;
        a.dc_out = w.dCrec[m][c]; a.lddc = R;
        a.ds = w.dS[m] + (size_t)i * 4 * R; a.ldds = K * 4 * R;
        a.dc_prev = w.dCrec[m][c ^ 1]; a.lddcp = R;
        a.dh_prev = nullptr; a.lddhp = 0;
        a.B = B; a.R = R; a.order = XG_ORDER_IFGO; a.mask_mode = XG_MASK_ZERO;
        a.drop = pos_drop(&nd, 0, 0);
        return a;
    };
    for (int i = K - 1; i >= 0; --i) {
        XG_TRY(xgk_lstm_bwd2(st, cell(0, i), cell(1, i)));
        c ^= 1;
        if (i > 0)
            for (int m = 0; m < 2; ++m)
                XG_TRY(product_nn(st, B, R, w.dHrec[m], R, false, w.dS[m] + (size_t)i * 4 * R, K * 4 * R, mo[m].whh, 4 * R, nullptr));
    }
    for (int m = 0; m < 2; ++m) {
        const int64_t n = (int64_t)BK * R;
        hipLaunchKernelGGL(pos_shift_h_kernel, dim3((unsigned)xg_cdiv64(n, POS_TPB)), dim3(POS_TPB), 0, st, w.Hcat, m, K, R, n, w.Hprev);
        XG_CHECK_LAUNCH();
        XG_TRY(wgrad(st, BK, 4 * R, R, w.dS[m], 4 * R, w.Hprev, R, gm[m].whh, gm[m].bih, gm[m].bhh));
        XG_TRY(wgrad(st, BK, 4 * R, R, w.dS[m], 4 * R, w.Xe[m], R, gm[m].wih, nullptr));
        XG_TRY(dgrad(st, BK, R, 4 * R, w.dS[m], 4 * R, mo[m].wih, w.dX, R, false));
        // BatchNorm + ReLU + dropout + frame mask backward (sub_modules.py:121-123, :204)
        XG_TRY(xgk_fill(st, w.bn_s1, 0.f, R));
        XG_TRY(xgk_fill(st, w.bn_s2, 0.f, R));
        XG_TRY(xgk_bn_bwd_reduce(st, w.dX, w.Xe[m], w.Z[m], w.mean[m], w.var[m], fm, BK, R, POS_BN_EPS,
                                 pos_drop(run, mo[m].site, 0), w.bn_s1, w.bn_s2));
        XG_TRY(xgk_bn_bwd_apply(st, w.dX, w.Z[m], w.mean[m], w.var[m], mo[m].bg, w.bn_s1, w.bn_s2, BK, R, POS_BN_EPS, run->train != 0,
                                gm[m].bb, gm[m].bg));
        XG_TRY(wgrad(st, BK, R, mo[m].F, w.dX, R, mo[m].feats, mo[m].F, gm[m].ew, gm[m].eb));
    }
    return XG_OK;
}

int backward(hipStream_t st, const XgpDims* d, const XgpParams* p, const XgpParams* g, const XgptRun* run, const float* fr,
             const float* fo, const float* fm, int Tp, const float* dlogp, const TWs& w, const float* dpos = nullptr) {
    const int B = d->B, K = d->K, R = d->R, A = d->A, E = d->E, C = d->C, T = d->T, BK = B * K, TB = Tp * B;
    const size_t BR = (size_t)B * R;
    pack_t(st, p->a2h_w, R, 4 * R, w.pkt_a2h);
    pack_t(st, p->h2h_w, R, 4 * R, w.pkt_h2h);
    pack_t(st, p->h2a_w, R, A, w.pkt_h2a);
    XG_CHECK_LAUNCH();
    // the gradient of the state behind step Tp - 1: zero, or what its consumer sends (include/xgate_pos_joint.h)
    if (dpos) {
        if (hipMemcpyAsync(w.dH[0], dpos, sizeof(float) * BR, hipMemcpyDeviceToDevice, st) != hipSuccess) return XG_EHIP;
    } else {
        XG_TRY(xgk_fill(st, w.dH[0], 0.f, (int64_t)BR));
    }
    XG_TRY(xgk_fill(st, w.dC, 0.f, (int64_t)BR));
    CellBwdArgs cb{};
    cb.dlogp = dlogp; cb.logit_w = p->logit_w; cb.new_mask = w.nm; cb.dc = w.dC;
    cb.B = B; cb.R = R; cb.C = C; cb.T = T; cb.Tp = Tp;
    int cur = 0;
    for (int t = Tp - 1; t >= 0; --t) {
        float* ds = w.DS + (size_t)t * B * 4 * R;
        float* dp = w.DP + (size_t)t * B * A;
        float* daf = w.DAF + t * BR;
        cb.t = t;
        cb.lp = w.LP + (size_t)t * B * C;
        cb.gates = w.GD + (size_t)t * B * 4 * R;
        cb.c_prev = w.Cst + t * BR; cb.c_out = w.Cst + (t + 1) * BR;
        cb.dh_in = w.dH[cur]; cb.dh_out = w.dH[cur ^ 1];
        cb.ds = ds; cb.dlogits = w.DLOG + (size_t)t * B * C;
        cb.drop = pos_drop(run, XG_SITE_L1, (uint32_t)t);
        hipLaunchKernelGGL(pos_cell_head_bwd_kernel, dim3(B), dim3(STEP_TPB), (size_t)C * sizeof(float), st, cb);
        XG_CHECK_LAUNCH();
        XG_TRY(product_nn(st, B, R, daf, R, false, ds, 4 * R, p->a2h_w, 4 * R, w.pkt_a2h));
        XG_TRY(xgk_attn_bwd(st, daf, R, w.P + (size_t)t * B * A, w.Q, w.V, p->a2w_w, w.ALPHA + (size_t)t * B * K,
                            w.DE + (size_t)t * B * K, dp, B, K, R, A));
        XG_TRY(product_nn(st, B, R, w.dH[cur ^ 1], R, true, ds, 4 * R, p->h2h_w, 4 * R, w.pkt_h2h, dp, A, p->h2a_w, A, w.pkt_h2a));
        cur ^= 1;
    }
    // batched parameter gradients over the T' B rows (row t B + b)
    XG_TRY(xgk_embed_gather(st, p->embed_w, E, w.cap, B, T, 1, TB, C, w.Xemb, E));
    XG_TRY(wgrad(st, TB, 4 * R, E, w.DS, 4 * R, w.Xemb, E, g->i2h_w, g->i2h_b, g->a2h_b, g->h2h_b));   // (the three folded biases)
    XG_TRY(wgrad(st, TB, 4 * R, R, w.DS, 4 * R, w.AF, R, g->a2h_w, nullptr));
    XG_TRY(wgrad(st, TB, 4 * R, R, w.DS, 4 * R, w.Hst, R, g->h2h_w, nullptr));
    XG_TRY(wgrad(st, TB, A, R, w.DP, A, w.Hst, R, g->h2a_w, g->h2a_b));
    XG_TRY(wgrad(st, TB, C, R, w.DLOG, C, w.Hst + BR, R, g->logit_w, g->logit_b));
    XG_TRY(dgrad(st, TB, E, 4 * R, w.DS, 4 * R, p->i2h_w, w.DXemb, E, false));
    XG_TRY(xgk_embed_scatter_add(st, g->embed_w, E, w.cap, B, T, 1, TB, C, w.DXemb, E));
    // attention after the loop: dV (plain store), d v2a(V) and a2w.weight; then v2a
    XG_TRY(xgk_attn_post_dV(st, w.P, w.Q, p->a2w_w, w.DE, w.DVPROJ, g->a2w_w, w.ALPHA, w.DAF, R, (int64_t)BR, w.DV, Tp, B, K, A, R));
    XG_TRY(wgrad(st, BK, A, R, w.DVPROJ, A, w.V, R, g->v2a_w, g->v2a_b));
    XG_TRY(dgrad(st, BK, R, A, w.DVPROJ, A, p->v2a_w, w.DV, R, true));
    // init_hidden: h0 / c0 = img_embed_{h,c}_1(vbar), vbar detached
    XG_TRY(wgrad(st, B, R, R, w.dH[cur], R, w.vbar, R, g->ih1_w, g->ih1_b));
    XG_TRY(wgrad(st, B, R, R, w.dC, R, w.vbar, R, g->ic1_w, g->ic1_b));
    return encoder_bwd(st, d, p, g, run, fr, fo, fm, w);
}

bool run_ok(const XgptRun* run) {
    return run && run->drop_p >= 0.f && run->drop_p < 1.f && run->bn_momentum >= 0.f && run->bn_momentum <= 1.f;
}

// the attention backward after the step loop (xgk_attn_post_dV -> xgk_attn_bwd_post) keeps a video's T x K score gradients in
// LDS and refuses more than XGPT_MAX_TK_BYTES of them: such shapes are refused here, before a forward moves the running
// statistics or a backward adds its first gradient
bool tk_ok(int64_t T, int64_t K) { return T * K * (int64_t)sizeof(float) <= XGPT_MAX_TK_BYTES; }

}  // namespace

extern "C" int xgpt_version(void) { return XGPT_VERSION; }

extern "C" size_t xgpt_workspace_bytes(const XgpDims* d) {
    if (!dims_ok(d, true) || !tk_ok(d->T, d->K)) return 0;
    return tws_layout(d, nullptr).floats * sizeof(float);
}

extern "C" int xgpt_forward_train(void* stream, const XgpDims* d, const XgpParams* p, const XgBnState* bn, const XgptRun* run,
                                  const float* feats_rgb, const float* feats_opfl, const float* feat_mask, const int64_t* cap_classes,
                                  const float* new_mask, float* logp, int32_t* t_out, void* ws, size_t ws_bytes) {
    if (!dims_ok(d, true) || !tk_ok(d->T, d->K) || !run_ok(run) || !cap_classes || !new_mask || !logp || !t_out) return XG_EINVAL;
    XG_TRY(args_gate(p, bn_ok(bn), feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, tws_layout(d, nullptr).floats));
    hipStream_t st = (hipStream_t)stream;
    XG_TRY(forward_train(st, d, p, bn, run, feats_rgb, feats_opfl, feat_mask, cap_classes, new_mask, logp, tws_layout(d, ws)));
    hipLaunchKernelGGL(pos_first_zero_col_kernel, dim3(1), dim3(POS_TPB), 0, st, cap_classes, nullptr, d->B, d->T, 0, t_out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

extern "C" int xgpt_backward(void* stream, const XgpDims* d, const XgpParams* p, const XgpParams* g, const XgptRun* run,
                             const float* feats_rgb, const float* feats_opfl, const float* feat_mask, int32_t Tp, const float* dlogp,
                             void* ws, size_t ws_bytes) {
    if (!dims_ok(d, true) || !params_ok(g) || !run_ok(run) || !dlogp || Tp < 1 || Tp > d->T || !tk_ok(Tp, d->K)) return XG_EINVAL;
    XG_TRY(args_gate(p, true, feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, tws_layout(d, nullptr).floats));   // (no running statistics)
    return backward((hipStream_t)stream, d, p, g, run, feats_rgb, feats_opfl, feat_mask, Tp, dlogp, tws_layout(d, ws));
}

// ---- joint training (include/xgate_pos_joint.h): the state the captioner consumes, and its gradient into the backward
extern "C" int xgpj_version(void) { return XGPJ_VERSION; }

extern "C" int xgpj_final_state(void* stream, const XgpDims* d, int32_t Tp, const void* ws, size_t ws_bytes, float* pos_feats) {
    if (!dims_ok(d, true) || !tk_ok(d->T, d->K) || Tp < 1 || Tp > d->T || !ws || !pos_feats) return XG_EINVAL;
    if (ws_bytes < tws_layout(d, nullptr).floats * sizeof(float)) return XG_EWORKSPACE;
    const TWs w = tws_layout(d, const_cast<void*>(ws));
    const size_t BR = (size_t)d->B * d->R;
    return hipMemcpyAsync(pos_feats, w.Hst + (size_t)Tp * BR, sizeof(float) * BR, hipMemcpyDeviceToDevice, (hipStream_t)stream) ==
                   hipSuccess ? XG_OK : XG_EHIP;
}

extern "C" int xgpj_backward(void* stream, const XgpDims* d, const XgpParams* p, const XgpParams* g, const XgptRun* run,
                             const float* feats_rgb, const float* feats_opfl, const float* feat_mask, int32_t Tp, const float* dlogp,
                             void* ws, size_t ws_bytes, const float* dpos) {
    if (!dims_ok(d, true) || !params_ok(g) || !run_ok(run) || (!dlogp && !dpos) || Tp < 1 || Tp > d->T || !tk_ok(Tp, d->K))
        return XG_EINVAL;
    XG_TRY(args_gate(p, true, feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, tws_layout(d, nullptr).floats));   // (no running statistics)
    return backward((hipStream_t)stream, d, p, g, run, feats_rgb, feats_opfl, feat_mask, Tp, dlogp, tws_layout(d, ws), dpos);
}

// ==================================================================================================================================
// Controlled generation (include/xgate_pos_control.h): the greedy rollout with the choice replaced by the caller's tag sequence, S
// templates for each of B videos.  The prologue (encoder, init_hidden, v2a(V), the token table, the packed weights) runs once over
// the B videos; one launch copies each video's initial h and c to its S rows (row b S + s); then the four launches of the step run
// over the M = B S rows: h2a, attention, a2h + h2h, cell + head.
//   attention      pos_attn_group_kernel: one workgroup per (video, group of CTRL_G templates).  Every row of the video's v2a(V) and
//                  V is fetched once and applied to each p-vector of the group, so the step reads the video's operands ceil(S / G)
//                  times instead of S times.  A row's scores and context sums are pos_attn_kernel's expressions in its order; its
//                  softmax is reduced by one wave (lane-strided partials, then the wave reduction) where pos_attn_kernel sums
//                  serially over k, so the two kernels may differ in the last bits.  Every row has one fixed order whatever group
//                  it falls in; S = 1 runs pos_attn_kernel itself, which is what makes that case bit-identical to the greedy call.
//   cell + head    pos_cell_head_rows_kernel<false>: the tag and the `unfinished` mask of the step from the template, the cell, then
//                  the log-sum-exp of the head and ONE gathered log-probability (the next tag's); no argmax.
// ==================================================================================================================================
#include "../../include/xgate_pos_control.h"

namespace {

constexpr int CTRL_G = XGPC_TEMPLATE_GROUP;

// the initial state of video b (X[b, R:2R], c[b]) to its S rows
__global__ void __launch_bounds__(POS_TPB) pos_bcast_state_kernel(const float* __restrict__ X, const float* __restrict__ c,
                                                                  float* __restrict__ X2, float* __restrict__ c2, int S, int R,
                                                                  int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * POS_TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / R, b = row / S;
    const int r = (int)(i - row * R);
    X2[row * 2 * R + R + r] = X[b * 2 * R + R + r];
    c2[i] = c[b * R + r];
}

// pos_attn_kernel for G templates of one video at a time: workgroup (b, group) serves rows b S + g0 .. + cnt - 1 (cnt < G in a
// video's last group when S % G != 0; the missing rows compute on zeros and store nothing).  P (M,A) and X (M,2R) are per row, Q
// (B,K,A) and V (B,K,R) per video.  The context parts take over the LDS of the p-vectors, which the scores are done with.
template <int G, bool V4>
__global__ void __launch_bounds__(STEP_TPB) pos_attn_group_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                                  const float* __restrict__ V, const float* __restrict__ w, float* X,
                                                                  int K, int R, int A, int S, int nsplit, int pr_floats) {
    extern __shared__ float lds[];
    float* ps = lds;                          // G x A, later red: nsplit x G x R
    float* red = lds;
    float* wsh = lds + pr_floats;             // A (pr_floats and the A below are rounded up to 4 floats: 16-byte rows for V4)
    float* al = wsh + (A + 3) / 4 * 4;        // G x K
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = (S + G - 1) / G;
    const int b = blockIdx.x / ng, g0 = (blockIdx.x - b * ng) * G;
    const int cnt = S - g0 < G ? S - g0 : G;
    const size_t row0 = (size_t)b * S + g0;
    const float* vb = V + (size_t)b * K * R;
    // (tests/test_gpu_pos_control.py: test_cases_reach_the_branches_they_name restates VREG, STEP_TPB and nsplit to pick a K past
    // the prefetch: change them together)
    constexpr int VREG = 16;
    const bool vpre = nsplit * R <= STEP_TPB && xg_cdiv_d(K, nsplit) <= VREG;
    const int vr = tid % R, vpart = tid / R;
    float vreg[VREG];
    if (vpre && tid < nsplit * R) {
#pragma unroll
        for (int i = 0; i < VREG; ++i) {
            const int k = vpart + i * nsplit;
            vreg[i] = k < K ? vb[(size_t)k * R + vr] : 0.f;
        }
    }
    for (int a = tid; a < A; a += STEP_TPB) {
        wsh[a] = w[a];
#pragma unroll
        for (int g = 0; g < G; ++g) ps[g * A + a] = g < cnt ? P[(row0 + g) * A + a] : 0.f;
    }
    __syncthreads();
    for (int k0 = wave; k0 < K; k0 += 2 * STEP_WAVES) {
        const int k1 = k0 + STEP_WAVES;
        const bool two = k1 < K;                                // wave-uniform
        const float* q0 = Q + ((size_t)b * K + k0) * A;
        const float* q1 = Q + ((size_t)b * K + (two ? k1 : k0)) * A;
        float acc0[G], acc1[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc0[g] = acc1[g] = 0.f;
        if (V4) {
            const float4* q04 = reinterpret_cast<const float4*>(q0);
            const float4* q14 = reinterpret_cast<const float4*>(q1);
            const float4* w4 = reinterpret_cast<const float4*>(wsh);
#pragma unroll 2
            for (int a4 = lane; a4 < A / 4; a4 += 64) {
                const float4 u = q04[a4];
                const float4 v = q14[a4];
                const float4 ww = w4[a4];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float4 pp = reinterpret_cast<const float4*>(ps + g * A)[a4];
                    acc0[g] += ww.x * xg_tanh(pp.x + u.x) + ww.y * xg_tanh(pp.y + u.y) + ww.z * xg_tanh(pp.z + u.z) +
                               ww.w * xg_tanh(pp.w + u.w);
                    acc1[g] += ww.x * xg_tanh(pp.x + v.x) + ww.y * xg_tanh(pp.y + v.y) + ww.z * xg_tanh(pp.z + v.z) +
                               ww.w * xg_tanh(pp.w + v.w);
                }
            }
        } else {
#pragma unroll 2
            for (int a = lane; a < A; a += 64) {
                const float u = q0[a], v = q1[a], ww = wsh[a];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float pp = ps[g * A + a];
                    acc0[g] += ww * xg_tanh(pp + u);
                    acc1[g] += ww * xg_tanh(pp + v);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float s0 = wave_sum(acc0[g]), s1 = wave_sum(acc1[g]);
            if (lane == 0) {
                al[g * K + k0] = s0;
                if (two) al[g * K + k1] = s1;
            }
        }
    }
    __syncthreads();
    // alpha = softmax_k(e), not masked: wave g normalises row g (a fixed order: lane-strided partials, then the wave reduction)
    if (wave < G) {
        float* ar = al + wave * K;
        float mx = -INFINITY;
        for (int k = lane; k < K; k += 64) mx = fmaxf(mx, ar[k]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += __expf(ar[k] - mx);
        s = wave_sum(s);
        for (int k = lane; k < K; k += 64) ar[k] = __expf(ar[k] - mx) / s;
    }
    __syncthreads();                                           // (alpha is final, and every wave is done with ps)
    if (vpre) {
        if (tid < nsplit * R) {
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.f;
#pragma unroll
            for (int i = 0; i < VREG; ++i) {
                const int k = vpart + i * nsplit;
                if (k < K) {
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[g] += al[g * K + k] * vreg[i];
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) red[(vpart * G + g) * R + vr] = acc[g];
        }
    } else {
        for (int i = tid; i < nsplit * R; i += STEP_TPB) {
            const int r = i % R, part = i / R;
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.f;
            for (int k = part; k < K; k += nsplit) {
                const float v = vb[(size_t)k * R + r];
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] += al[g * K + k] * v;
            }
#pragma unroll
            for (int g = 0; g < G; ++g) red[(part * G + g) * R + r] = acc[g];
        }
    }
    __syncthreads();
    for (int i = tid; i < cnt * R; i += STEP_TPB) {
        const int g = i / R, r = i - g * R;
        float acc = red[g * R + r];
        for (int part = 1; part < nsplit; ++part) acc += red[(part * G + g) * R + r];
        X[(row0 + g) * 2 * R + r] = acc;
    }
}

struct RowsArgs {
    const float* S;              // (M,4R) af a2h^T + h h2h^T, no bias
    const float* tab;            // (C,4R) embed i2h^T + the three biases
    const float *logit_w, *logit_b;
    float* X;                    // (M,2R): h read from and h' written to columns R..2R
    float* c;                    // (M,R) cell state, in place
    const int64_t* tmpl;         // (M,T-1) the tags: column t - 1 is read by step t
    float *tag_logp, *states, *masks, *pos_feats;   // (M,T-1), (M,T,R) or null, (M,T), (M,R)
    // DRAW only: tmpl_out is tmpl, writable (step t writes column t); one uniform per row and step
    int64_t* tmpl_out;
    const float* uniforms;       // (M,T-1)
    float temperature;
    int R, C, T, t;
};

// inclusive scan over the 64 lanes: row_shr 1, 2, 4, 8 inside each row of 16 (zeros shift in), then the totals of the rows before
// the lane's own, added in row order.  Every lane must be active.
__device__ __forceinline__ float wave_scan(float v) {
    v += xg_dpp<0x111>(v);
    v += xg_dpp<0x112>(v);
    v += xg_dpp<0x114>(v);
    v += xg_dpp<0x118>(v);
    const float r0 = xg_readlane(v, 15), r1 = xg_readlane(v, 31), r2 = xg_readlane(v, 47);
    const int row = (threadIdx.x & 63) >> 4;
    const float before = row == 0 ? 0.f : (row == 1 ? r0 : (row == 2 ? r0 + r1 : (r0 + r1) + r2));
    return before + v;
}

// one workgroup per row, step t: the tag fed is tmpl[t-1] (BOS at t = 0) under the mask unfinished_t = unfinished_{t-1} (tag > 0)
// (unfinished_{t-1} is masks[t-1], written by the step before); the cell; then, for t < T - 1, the head's log-sum-exp and the
// log-probability of the NEXT tag, which counts while the row is unfinished at step t: up to and including its first 0.
//   !DRAW  the next tag is the caller's tmpl[t].
//   DRAW   it is drawn here and written to tmpl_out[t], where the launch of step t + 1 reads it: the first category whose running
//          sum of w_c = exp((x_c - max x) / temperature) exceeds uniforms[t] * sum(w), C - 1 when none does (the captioner's draw,
//          xg_select.h).  tmpl_out[t] = tag * unfinished; tag_logp[t] is the UNtempered log-probability of the tag.
template <bool DRAW>
__global__ void __launch_bounds__(STEP_TPB) pos_cell_head_rows_kernel(RowsArgs a) {
    extern __shared__ float lds[];
    float* hs = lds;             // R
    float* lg = lds + a.R;       // C
    float* wt = lg + a.C;        // C, DRAW only (the serial head's weights)
    const int tid = threadIdx.x, R = a.R, C = a.C, T = a.T, t = a.t;
    const size_t row = blockIdx.x;
    const int64_t* tr = a.tmpl + row * (T - 1);
    int64_t tk = 0;
    float m = 1.0f;
    if (t > 0) {
        tk = pos_clamp_tag(tr[t - 1], C);
        m = tk > 0 ? a.masks[row * T + t - 1] : 0.0f;
    }
    const float* s = a.S + row * 4 * R;
    const float* tb = a.tab + (size_t)tk * 4 * R;
    float* xh = a.X + row * 2 * R + R;
    float* cb = a.c + row * R;
    float* st = a.states ? a.states + (row * T + t) * R : nullptr;
    float* pf = t == T - 1 ? a.pos_feats + row * R : nullptr;
    for (int j = tid; j < R; j += STEP_TPB) {
        const PosCell o = pos_cell(s, tb, R, j, cb[j], xh[j], m);
        cb[j] = o.cn;
        xh[j] = o.hn;
        hs[j] = o.hn;
        if (st) st[j] = o.hn;
        if (pf) pf[j] = o.hn;
    }
    if (tid == 0) a.masks[row * T + t] = m;
    if (t + 1 >= T) return;                                     // (no tag follows the last step)
    const float u = DRAW ? a.uniforms[row * (T - 1) + t] : 0.f;   // (requested here: the head's products hide the round trip)
    pos_head_logits(a.logit_w, a.logit_b, hs, lg, R, C);
    const int lane = tid & 63, wave = tid >> 6;
    int nx = DRAW ? C - 1 : (int)pos_clamp_tag(tr[t], C);   // DRAW: stays when nothing passes the target (rounding, u = 1)
    float mx, lse = 0.f;
    if (C <= 64) {                                              // one lane per category
        if (wave == 0) {
            const float v = lane < C ? lg[lane] : -INFINITY;
            lse = pos_lse_lanes(v, lane < C, mx);
            if (DRAW) {
                const float inc = wave_scan(lane < C ? expf((v - mx) / a.temperature) : 0.f);
                const float target = u * xg_readlane(inc, C - 1);     // (the total in the last category's own summation order)
                const unsigned long long pass = __ballot(lane < C && inc > target);
                if (pass) nx = __ffsll(pass) - 1;
            }
        }
    } else if (tid == 0) {
        lse = pos_lse_serial(lg, C, mx);
        if (DRAW) {
            float tot = 0.f;
            for (int cc = 0; cc < C; ++cc) {
                wt[cc] = expf((lg[cc] - mx) / a.temperature);
                tot += wt[cc];
            }
            const float target = u * tot;
            float run = 0.f;
            for (int cc = 0; cc < C; ++cc) {
                run += wt[cc];
                if (run > target) { nx = cc; break; }
            }
        }
    }
    if (tid == 0) {                                             // (the thread that holds lse and nx in both forms)
        a.tag_logp[row * (T - 1) + t] = m != 0.0f ? lg[nx] - lse : 0.0f;
        if (DRAW) a.tmpl_out[row * (T - 1) + t] = m != 0.0f ? nx : 0;
    }
}

// the workspace: xgp's regions for the B videos, then the step's operands for the M = B S rows
struct CWs {
    Ws v;
    float *X, *P, *S, *c;
    size_t floats;
};

CWs cws_layout(const XgpDims* d, int S, void* base) {
    CWs w;
    w.v = ws_layout(d, base);
    const size_t M = (size_t)d->B * S, R = d->R, A = d->A;
    Carve cv{(float*)base, w.v.floats};
    w.X = cv.take(M * 2 * R);           // [af ; h] of every row
    w.P = cv.take(M * A);
    w.S = cv.take(M * 4 * R);
    w.c = cv.take(M * R);
    w.floats = cv.off;
    return w;
}

// LDS floats of pos_attn_group_kernel<G>: the p-vectors / context parts, w, the scores
// (restated as group_lds in tests/test_gpu_pos_control.py, with the 64 KiB limit of step_plan below, to name the cases that take
// the one-template form: change them together)
size_t attn_group_lds(int G, int K, int R, int A, int nsplit, int* pr_floats) {
    const size_t pr = ((size_t)G * (A > nsplit * R ? A : nsplit * R) + 3) / 4 * 4;
    *pr_floats = (int)pr;
    return (pr + (size_t)(A + 3) / 4 * 4 + (size_t)G * K) * sizeof(float);
}

bool ctrl_dims_ok(const XgpDims* d, int S) {
    if (!dims_ok(d, true) || d->T < 2 || S < 1) return false;
    const int64_t M = (int64_t)d->B * S;
    // (A, R <= 4096: 32-bit row offsets into the (M, .) operands, and the (M,T,R) states)
    return M * 4 * 4096 < (1LL << 31) && M * d->T * d->R < (1LL << 31);
}

StepPlan step_plan(const XgpDims* d, int S) {
    const int K = d->K, R = d->R, A = d->A;
    StepPlan pl{};
    pl.S = S;
    pl.v4 = A % 4 == 0;
    // the context parts of pos_attn_kernel / pos_attn_group_kernel: as many as fill the workgroup, at most one per frame
    pl.nsplit = STEP_TPB / R < 1 ? 1 : (STEP_TPB / R > K ? K : STEP_TPB / R);
    if (S == 1) {                // pos_attn_kernel itself: what makes a one-row call bit-identical to the greedy one
        pl.lds = (size_t)(2 * A + K + pl.nsplit * R) * sizeof(float);
        return pl;
    }
    // the full group while it fits the 64 KiB of LDS a workgroup gets without opting in; else (A or R near 4096) one template
    pl.G = CTRL_G;
    pl.lds = attn_group_lds(CTRL_G, K, R, A, pl.nsplit, &pl.pr_floats);
    if (pl.lds > 64 * 1024) {
        pl.G = 1;
        pl.lds = attn_group_lds(1, K, R, A, pl.nsplit, &pl.pr_floats);
    }
    return pl;
}

template <int G>
void launch_attn_group(hipStream_t st, int B, const StepPlan& pl, const float* P, const float* Q, const float* V, const float* w,
                       float* X, int K, int R, int A) {
    const dim3 grid(B * xg_cdiv(pl.S, G)), tpb(STEP_TPB);
    if (pl.v4) hipLaunchKernelGGL((pos_attn_group_kernel<G, true>), grid, tpb, pl.lds, st, P, Q, V, w, X, K, R, A, pl.S, pl.nsplit, pl.pr_floats);
    else       hipLaunchKernelGGL((pos_attn_group_kernel<G, false>), grid, tpb, pl.lds, st, P, Q, V, w, X, K, R, A, pl.S, pl.nsplit, pl.pr_floats);
}

int step_front(hipStream_t st, const XgpDims* d, const XgpParams* p, const StepPlan& pl, const Ws& v, float* X, float* P, float* S) {
    const int B = d->B, K = d->K, R = d->R, A = d->A, M = B * pl.S;
    const float* w = p->a2w_w;
    XG_TRY(product(st, M, A, X + R, 2 * R, p->h2a_w, R, nullptr, 0, nullptr, 0, p->h2a_b, P, A, false, v.pk_h2a));
    if (pl.G == CTRL_G) launch_attn_group<CTRL_G>(st, B, pl, P, v.Q, v.V, w, X, K, R, A);
    else if (pl.G == 1) launch_attn_group<1>(st, B, pl, P, v.Q, v.V, w, X, K, R, A);
    else launch_attn(st, B, pl, P, v.Q, v.V, w, X, K, R, A);
    XG_CHECK_LAUNCH();
    return product(st, M, 4 * R, X, 2 * R, p->a2h_w, R, X + R, 2 * R, p->h2h_w, R, nullptr, S, 4 * R, false, v.pk_a2h, v.pk_h2h);
}

// the prologue over the B videos, then each video's initial h and c copied to its S rows
int rows_prologue(hipStream_t st, const XgpDims* d, int S, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo,
                  const float* fm, const CWs& w) {
    XG_TRY(prologue(st, d, p, bn, fr, fo, fm, w.v));
    const int64_t n = (int64_t)d->B * S * d->R;
    hipLaunchKernelGGL(pos_bcast_state_kernel, dim3((unsigned)xg_cdiv(n, POS_TPB)), dim3(POS_TPB), 0, st, w.v.X, w.v.c, w.X, w.c, S, d->R, n);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// the rollout over the M = B S rows (fa: the caller's operands; the workspace's and the step are filled in here), then n_out from
// the masks.  `draw` picks pos_cell_head_rows_kernel<true>, which needs C more floats of LDS for the weights of its serial head.
int rollout_rows(hipStream_t st, const XgpDims* d, int S, const XgpParams* p, const XgBnState* bn, const float* fr, const float* fo,
                 const float* fm, RowsArgs fa, bool draw, int32_t* n_out, const CWs& w) {
    const int R = d->R, C = d->C, T = d->T, M = d->B * S;
    XG_TRY(rows_prologue(st, d, S, p, bn, fr, fo, fm, w));
    fa.S = w.S; fa.tab = w.v.tab; fa.logit_w = p->logit_w; fa.logit_b = p->logit_b;
    fa.X = w.X; fa.c = w.c; fa.R = R; fa.C = C; fa.T = T;
    const size_t lds_cell = (size_t)(R + (draw ? 2 : 1) * C) * sizeof(float);
    const StepPlan pl = step_plan(d, S);
    for (int t = 0; t < T; ++t) {
        XG_TRY(step_front(st, d, p, pl, w.v, w.X, w.P, w.S));
        fa.t = t;
        if (draw) hipLaunchKernelGGL(pos_cell_head_rows_kernel<true>, dim3(M), dim3(STEP_TPB), lds_cell, st, fa);
        else      hipLaunchKernelGGL(pos_cell_head_rows_kernel<false>, dim3(M), dim3(STEP_TPB), lds_cell, st, fa);
        XG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pos_first_zero_col_kernel, dim3(1), dim3(POS_TPB), 0, st, nullptr, fa.masks, M, T, 1, n_out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

}  // namespace

extern "C" int xgpc_version(void) { return XGPC_VERSION; }

extern "C" size_t xgpc_workspace_bytes(const XgpDims* d, int32_t S) {
    if (!ctrl_dims_ok(d, S)) return 0;
    return cws_layout(d, S, nullptr).floats * sizeof(float);
}

extern "C" int xgpc_sample_forced(void* stream, const XgpDims* d, int32_t S, const XgpParams* p, const XgBnState* bn,
                                  const float* feats_rgb, const float* feats_opfl, const float* feat_mask, const int64_t* templates,
                                  float* tag_logp, float* states, float* masks, float* pos_feats, int32_t* n_out, void* ws,
                                  size_t ws_bytes) {
    if (!ctrl_dims_ok(d, S) || !templates || !tag_logp || !masks || !pos_feats || !n_out) return XG_EINVAL;
    XG_TRY(args_gate(p, bn_ok(bn), feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, cws_layout(d, S, nullptr).floats));
    RowsArgs fa{};
    fa.tmpl = templates; fa.tag_logp = tag_logp; fa.states = states; fa.masks = masks; fa.pos_feats = pos_feats;
    return rollout_rows((hipStream_t)stream, d, S, p, bn, feats_rgb, feats_opfl, feat_mask, fa, false, n_out, cws_layout(d, S, ws));
}

// ==================================================================================================================================
// Sampled templates (include/xgate_pos_sample.h): the forced rollout above with the tag of step t + 1 DRAWN at the end of step t
// from the head's distribution and written to `templates`, where the next step's launch reads it as the forced call reads the
// caller's.  The same rollout_rows and workspace; the step's fourth launch is pos_cell_head_rows_kernel<true>.
// ==================================================================================================================================
#include "../../include/xgate_pos_sample.h"

extern "C" int xgps_version(void) { return XGPS_VERSION; }

extern "C" size_t xgps_workspace_bytes(const XgpDims* d, int32_t S) { return xgpc_workspace_bytes(d, S); }

extern "C" int xgps_sample_templates(void* stream, const XgpDims* d, int32_t S, float temperature, const XgpParams* p,
                                     const XgBnState* bn, const float* feats_rgb, const float* feats_opfl, const float* feat_mask,
                                     const float* uniforms, int64_t* templates, float* tag_logp, float* states, float* masks,
                                     float* pos_feats, int32_t* n_out, void* ws, size_t ws_bytes) {
    if (!ctrl_dims_ok(d, S) || !(temperature > 0.0f) || temperature == INFINITY || !uniforms || !templates || !tag_logp || !masks ||
        !pos_feats || !n_out)
        return XG_EINVAL;
    XG_TRY(args_gate(p, bn_ok(bn), feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, cws_layout(d, S, nullptr).floats));
    RowsArgs sa{};
    sa.tmpl = templates; sa.tag_logp = tag_logp; sa.states = states; sa.masks = masks; sa.pos_feats = pos_feats;
    sa.tmpl_out = templates; sa.uniforms = uniforms; sa.temperature = temperature;
    return rollout_rows((hipStream_t)stream, d, S, p, bn, feats_rgb, feats_opfl, feat_mask, sa, true, n_out, cws_layout(d, S, ws));
}

// ==================================================================================================================================
// Beam templates (include/xgate_pos_beam.h): the beam search of pos_src/SAModel.py:104-134 / pos_src/CaptionModel.py:22-125, W slots
// for each of B videos, rows b W + slot.  The prologue with the copy of the initial state (rows_prologue) and the first three launches
// of the step (step_front) are rollout_rows' own, over the M = B W rows (a video's W beams are one attention group).  The fourth launch is
// pos_beam_merge_kernel, ONE workgroup per video: the C-way head is small enough that the whole merge of a video (W rows of C
// log-probabilities, W * W candidates) fits in one workgroup, so no step needs the host.
//   1. pos_cell of all W rows into LDS (mask 1: dead slots keep running, as the reference's get_logprobs_state does); every c and h
//      of the step before is read here, before anything is written.
//   2. pos_head_logits per row, pos_lse_* per row (wave q serves row q), the -1000 on `suppress_tag`.
//   3. per row the W largest log-probabilities in descending order, lower category first on ties, into the candidate tables:
//      C <= 64 by counting (one lane per category), beyond by lane 0 of the row's wave serially.
//   4. beam_merge (xg_beam_core.h): the rest of step 3 and steps 4-5 of the rule, shared with the captioner's search.
//   5. every thread: h and c of slot v from parent q out of LDS.  The rows are this workgroup's alone: barrier, then write.
// pos_beam_backtrace_kernel then follows each done entry's parents back (beam_backtrace_row) and appends the masks, and
// pos_first_zero_col_kernel writes n_out.
// ==================================================================================================================================
#include "../../include/xgate_pos_beam.h"

namespace {

constexpr int BEAM_MAX = XG_BEAM_MAX;
static_assert(BEAM_MAX <= STEP_WAVES, "one wave per row of the video");

struct BeamArgs {
    const float* S;              // (M,4R) af a2h^T + h h2h^T, no bias
    const float* tab;            // (C,4R) embed i2h^T + the three biases
    const float *logit_w, *logit_b;
    float* X;                    // (M,2R): h read from and h' written to columns R..2R
    float* c;                    // (M,R) cell state, in place
    BeamBook<int32_t> book;
    int R, C, suppress;
};

__global__ void __launch_bounds__(STEP_TPB) pos_beam_merge_kernel(BeamArgs a) {
    extern __shared__ float lds[];
    __shared__ BeamTables T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, C = a.C, W = a.book.W, t = a.book.t;
    const size_t b = blockIdx.x, row0 = b * W;
    float* hs = lds;                          // W x R
    float* cs = hs + (size_t)W * R;           // W x R
    float* lg = cs + (size_t)W * R;           // W x C: the logits, then the log-probabilities
    // (a NaN ranks nowhere: whatever stays unwritten below is category 0, never an index out of range)
    if (tid < BEAM_MAX * BEAM_MAX) { T.c_lp[tid] = 0.f; T.c_tok[tid] = 0; }
    for (int i = tid; i < W * R; i += STEP_TPB) {
        const int q = i / R, j = i - q * R;
        const size_t row = row0 + q;
        const int64_t tk = t == 0 ? 0 : pos_clamp_tag(a.book.tok[row], C);
        const PosCell o = pos_cell(a.S + row * 4 * R, a.tab + (size_t)tk * 4 * R, R, j, a.c[row * R + j], a.X[row * 2 * R + R + j], 1.0f);
        hs[i] = o.hn;
        cs[i] = o.cn;
    }
    const int rows = t == 0 ? 1 : W;          // (every slot holds the video's initial state at t = 0)
    for (int q = 0; q < rows; ++q) pos_head_logits(a.logit_w, a.logit_b, hs + (size_t)q * R, lg + (size_t)q * C, R, C);
    if (wave < rows) {                        // wave q: the log-probabilities of row q, in place
        float* lr = lg + (size_t)wave * C;
        float mx;
        if (C <= 64) {
            const float v = lane < C ? lr[lane] : -INFINITY;
            const float lse = pos_lse_lanes(v, lane < C, mx);
            float lp = v - lse;
            if (lane == a.suppress) lp -= 1000.0f;
            if (lane < C) lr[lane] = lp;
        } else if (lane == 0) {
            const float lse = pos_lse_serial(lr, C, mx);
            for (int cc = 0; cc < C; ++cc) lr[cc] -= lse;
            if (a.suppress >= 0) lr[a.suppress] -= 1000.0f;
        }
    }
    __syncthreads();
    if (wave < rows) {                        // the W largest of row q, descending, lower category first on ties (the gate: W <= C)
        const float* lr = lg + (size_t)wave * C;
        if (C <= 64) {
            if (lane < C) {
                const float me = lr[lane];
                int rank = 0;
                for (int cc = 0; cc < C; ++cc) rank += beam_before(lr[cc], cc, me, lane) ? 1 : 0;
                if (rank < W) { T.c_lp[wave * BEAM_MAX + rank] = me; T.c_tok[wave * BEAM_MAX + rank] = lane; }
            }
        } else if (lane == 0) {
            float pv = INFINITY;
            int pc = -1;
            for (int k = 0; k < W; ++k) {     // the largest of what comes after the pick before in that order
                float bv = 0.f;
                int bc = -1;
                for (int cc = 0; cc < C; ++cc) {
                    const float o = lr[cc];
                    if (beam_before(pv, pc, o, cc) && (bc < 0 || o > bv)) { bv = o; bc = cc; }
                }
                if (bc < 0) break;
                T.c_lp[wave * BEAM_MAX + k] = bv;
                T.c_tok[wave * BEAM_MAX + k] = bc;
                pv = bv;
                pc = bc;
            }
        }
    }
    beam_merge(T, a.book, b, rows);
    for (int i = tid; i < W * R; i += STEP_TPB) {
        const int v = i / R, j = i - v * R;
        const int q = T.s_q[v];
        a.X[(row0 + v) * 2 * R + R + j] = hs[(size_t)q * R + j];
        a.c[(row0 + v) * R + j] = cs[(size_t)q * R + j];
    }
}

// one thread per (video, rank): the done entry's beam, read back along its parents
__global__ void __launch_bounds__(POS_TPB) pos_beam_backtrace_kernel(BeamBook<int32_t> k, int64_t* templates, float* tag_logp,
                                                                     float* score, float* masks, int M) {
    const int i = blockIdx.x * POS_TPB + threadIdx.x;
    if (i >= M) return;
    const int L = k.L;
    beam_backtrace_row(k, i, templates, tag_logp, score);
    const int64_t* tm = templates + (size_t)i * L;
    float* mk = masks + (size_t)i * (L + 1);
    float m = 1.0f;
    mk[0] = m;
    for (int t = 1; t <= L; ++t) {
        if (tm[t - 1] == 0) m = 0.0f;
        mk[t] = m;
    }
}

// the workspace: the forced call's at S = W, then the search's own regions
struct BWs {
    CWs c;
    BeamBook<int32_t> book;
    size_t floats;
};

BWs bws_layout(const XgpDims* d, int W, void* base) {
    BWs w;
    w.c = cws_layout(d, W, base);
    Carve cv{(float*)base, w.c.floats};
    w.book = beam_book_carve<int32_t>(cv, d->B, W, d->T - 1);
    w.floats = cv.off;
    return w;
}

bool beam_dims_ok(const XgpDims* d, int W, int suppress) {
    if (!ctrl_dims_ok(d, W < 1 ? 1 : W)) return false;
    if (W < 1 || W > BEAM_MAX || W > d->C || suppress >= d->C) return false;
    return XGPB_LDS_BYTES(W, d->R, d->C) <= XGPB_MAX_LDS_BYTES;
}

}  // namespace

extern "C" int xgpb_version(void) { return XGPB_VERSION; }

extern "C" size_t xgpb_workspace_bytes(const XgpDims* d, int32_t W) {
    if (!beam_dims_ok(d, W, -1)) return 0;
    return bws_layout(d, W, nullptr).floats * sizeof(float);
}

extern "C" int xgpb_beam_templates(void* stream, const XgpDims* d, int32_t W, int32_t suppress_tag, const XgpParams* p,
                                   const XgBnState* bn, const float* feats_rgb, const float* feats_opfl, const float* feat_mask,
                                   int64_t* templates, float* tag_logp, float* score, float* masks, int32_t* n_out, int32_t* trace,
                                   void* ws, size_t ws_bytes) {
    if (!beam_dims_ok(d, W, suppress_tag) || !templates || !tag_logp || !score || !masks || !n_out) return XG_EINVAL;
    XG_TRY(args_gate(p, bn_ok(bn), feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, bws_layout(d, W, nullptr).floats));
    hipStream_t st = (hipStream_t)stream;
    const BWs w = bws_layout(d, W, ws);
    const int B = d->B, R = d->R, C = d->C, L = d->T - 1, M = B * W;
    XG_TRY(rows_prologue(st, d, W, p, bn, feats_rgb, feats_opfl, feat_mask, w.c));
    BeamArgs a{};
    a.S = w.c.S; a.tab = w.c.v.tab; a.logit_w = p->logit_w; a.logit_b = p->logit_b; a.X = w.c.X; a.c = w.c.c;
    a.book = w.book; a.book.trace_out = trace;
    a.R = R; a.C = C; a.suppress = suppress_tag < 0 ? -1 : suppress_tag;
    const size_t lds_merge = XGPB_LDS_BYTES(W, R, C) - 1024;
    const StepPlan pl = step_plan(d, W);         // (a video's W beams are one attention group)
    for (int t = 0; t < L; ++t) {
        XG_TRY(step_front(st, d, p, pl, w.c.v, w.c.X, w.c.P, w.c.S));
        a.book.t = t;
        hipLaunchKernelGGL(pos_beam_merge_kernel, dim3(B), dim3(STEP_TPB), lds_merge, st, a);
        XG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pos_beam_backtrace_kernel, dim3(xg_cdiv(M, POS_TPB)), dim3(POS_TPB), 0, st, w.book, templates, tag_logp,
                       score, masks, M);
    XG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pos_first_zero_col_kernel, dim3(1), dim3(POS_TPB), 0, st, nullptr, masks, M, L + 1, 1, n_out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}

// ==================================================================================================================================
// Diverse beam templates (include/xgate_pos_beam_diverse.h): Gd groups of Wg slots per video, N = Gd Wg rows, each group a beam search
// of width Wg, the groups of a video merged in series within a step under the Hamming penalty of the earlier groups' live new tags
// (the group form of xg_beam_core.h).  The launches are the plain search's at W = N; the step's fourth launch is
// pos_beam_merge_diverse_kernel, ONE workgroup per video: the plain merge kernel's cell, head and log-sum-exp over the video's N rows,
// then per group the re-rank of its rows' full C-way log-probabilities (they sit in LDS, so the penalty is applied to them directly)
// and beam_group_merge, then every slot's h and c from its parent.  The book is carved as (B Gd, Wg, L): the backtrace is the plain one.
// ==================================================================================================================================
#include "../../include/xgate_pos_beam_diverse.h"

namespace {

static_assert(sizeof(BeamGroupTables) + 128 <= 1536, "the fixed part of XGPD_LDS_BYTES (1536) holds the group tables");

__global__ void __launch_bounds__(STEP_TPB) pos_beam_merge_diverse_kernel(BeamArgs a, int Gd, float lambda) {
    extern __shared__ float lds[];
    __shared__ BeamGroupTables G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, C = a.C, Wg = a.book.W, N = Gd * Wg, t = a.book.t;
    const size_t b = blockIdx.x, row0 = b * N;
    float* hs = lds;                          // N x R
    float* cs = hs + (size_t)N * R;           // N x R
    float* lg = cs + (size_t)N * R;           // N x C: the logits, then the log-probabilities
    beam_group_begin(G);
    for (int i = tid; i < N * R; i += STEP_TPB) {
        const int q = i / R, j = i - q * R;
        const size_t row = row0 + q;
        const int64_t tk = t == 0 ? 0 : pos_clamp_tag(a.book.tok[row], C);
        const PosCell o = pos_cell(a.S + row * 4 * R, a.tab + (size_t)tk * 4 * R, R, j, a.c[row * R + j], a.X[row * 2 * R + R + j], 1.0f);
        hs[i] = o.hn;
        cs[i] = o.cn;
    }
    const int rows = t == 0 ? 1 : N;          // (every slot holds the video's initial state at t = 0: row 0 stands for each group's)
    for (int q = 0; q < rows; ++q) pos_head_logits(a.logit_w, a.logit_b, hs + (size_t)q * R, lg + (size_t)q * C, R, C);
    if (wave < rows) {                        // wave q: the log-probabilities of row q, in place
        float* lr = lg + (size_t)wave * C;
        float mx;
        if (C <= 64) {
            const float v = lane < C ? lr[lane] : -INFINITY;
            const float lse = pos_lse_lanes(v, lane < C, mx);
            float lp = v - lse;
            if (lane == a.suppress) lp -= 1000.0f;
            if (lane < C) lr[lane] = lp;
        } else if (lane == 0) {
            const float lse = pos_lse_serial(lr, C, mx);
            for (int cc = 0; cc < C; ++cc) lr[cc] -= lse;
            if (a.suppress >= 0) lr[a.suppress] -= 1000.0f;
        }
    }
    __syncthreads();
    const int grows = t == 0 ? 1 : Wg;
    for (int j = 0; j < Gd; ++j) {            // the groups in series: group j sees the live new tags of groups 0 .. j-1
        if (wave < grows) beam_group_rerank(G, wave, lg + (size_t)(t == 0 ? 0 : j * Wg + wave) * C, nullptr, C, C - 1, Wg, lambda, lane);
        beam_group_merge(G, a.book, b, Gd, j, grows);
    }
    for (int i = tid; i < N * R; i += STEP_TPB) {
        const int v = i / R, j = i - v * R;
        const int q = G.par[v];
        a.X[(row0 + v) * 2 * R + R + j] = hs[(size_t)q * R + j];
        a.c[(row0 + v) * R + j] = cs[(size_t)q * R + j];
    }
}

// the workspace: the forced call's at S = N, then the book of the B Gd groups
BWs dws_layout(const XgpDims* d, int Gd, int Wg, void* base) {
    BWs w;
    w.c = cws_layout(d, Gd * Wg, base);
    Carve cv{(float*)base, w.c.floats};
    w.book = beam_book_carve<int32_t>(cv, (size_t)d->B * Gd, Wg, d->T - 1);
    w.floats = cv.off;
    return w;
}

bool diverse_dims_ok(const XgpDims* d, int Gd, int Wg, int suppress) {
    if (Gd < 1 || Wg < 1 || Gd > BEAM_MAX || Wg > BEAM_MAX || Gd * Wg > BEAM_MAX) return false;
    const int N = Gd * Wg;
    if (!ctrl_dims_ok(d, N) || N > d->C || suppress >= d->C) return false;
    return XGPD_LDS_BYTES(N, d->R, d->C) <= XGPD_MAX_LDS_BYTES;
}

}  // namespace

extern "C" int xgpd_version(void) { return XGPD_VERSION; }

extern "C" size_t xgpd_workspace_bytes(const XgpDims* d, int32_t Gd, int32_t Wg) {
    if (!diverse_dims_ok(d, Gd, Wg, -1)) return 0;
    return dws_layout(d, Gd, Wg, nullptr).floats * sizeof(float);
}

extern "C" int xgpd_beam_templates(void* stream, const XgpDims* d, int32_t Gd, int32_t Wg, float lambda, int32_t suppress_tag,
                                   const XgpParams* p, const XgBnState* bn, const float* feats_rgb, const float* feats_opfl,
                                   const float* feat_mask, int64_t* templates, float* tag_logp, float* score, float* masks,
                                   int32_t* n_out, int32_t* trace, void* ws, size_t ws_bytes) {
    if (!diverse_dims_ok(d, Gd, Wg, suppress_tag) || !(lambda >= 0.0f) || lambda == INFINITY || !templates || !tag_logp || !score ||
        !masks || !n_out)
        return XG_EINVAL;
    XG_TRY(args_gate(p, bn_ok(bn), feats_rgb, feats_opfl, feat_mask, ws, ws_bytes, dws_layout(d, Gd, Wg, nullptr).floats));
    hipStream_t st = (hipStream_t)stream;
    const BWs w = dws_layout(d, Gd, Wg, ws);
    const int B = d->B, R = d->R, C = d->C, L = d->T - 1, N = Gd * Wg, M = B * N;
    XG_TRY(rows_prologue(st, d, N, p, bn, feats_rgb, feats_opfl, feat_mask, w.c));
    BeamArgs a{};
    a.S = w.c.S; a.tab = w.c.v.tab; a.logit_w = p->logit_w; a.logit_b = p->logit_b; a.X = w.c.X; a.c = w.c.c;
    a.book = w.book; a.book.trace_out = trace;
    a.R = R; a.C = C; a.suppress = suppress_tag < 0 ? -1 : suppress_tag;
    const size_t lds_merge = XGPD_LDS_BYTES(N, R, C) - 1536;
    const StepPlan pl = step_plan(d, N);         // (a video's N slots are one attention group)
    for (int t = 0; t < L; ++t) {
        XG_TRY(step_front(st, d, p, pl, w.c.v, w.c.X, w.c.P, w.c.S));
        a.book.t = t;
        hipLaunchKernelGGL(pos_beam_merge_diverse_kernel, dim3(B), dim3(STEP_TPB), lds_merge, st, a, Gd, lambda);
        XG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pos_beam_backtrace_kernel, dim3(xg_cdiv(M, POS_TPB)), dim3(POS_TPB), 0, st, w.book, templates, tag_logp,
                       score, masks, M);
    XG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pos_first_zero_col_kernel, dim3(1), dim3(POS_TPB), 0, st, nullptr, masks, M, L + 1, 1, n_out);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
