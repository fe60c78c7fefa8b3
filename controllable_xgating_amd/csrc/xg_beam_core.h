// The merge rule of both on-device beam searches, once: the captioner's (xg_beam.hip, include/xgate_beam.h) and the POS
// generator's (xg_pos.hip, include/xgate_pos_beam.h).  Steps 1-2 of those headers (the decoder step and the log-probabilities) and
// the first half of step 3 (each row's W best) are the caller's; what follows them is the same for both and lives here.
// One workgroup per video; c_lp / c_tok [q * XG_BEAM_MAX + k] hold row q's k-th best log-probability and its token, lower token
// first on exact ties, for q < rows (1 at t = 0, else W) and k < W.  That every row HAS W entries is the gate's job: it refuses
// W > V (captioner) and W > C (POS).
//   3. candidate c_rank * rows + q carries p = sum[q] + lp (one fp32 add); the <= 64 candidates are ranked by counting in the
//      order of beam_before (stable: lower index first on ties) and the first W are the new slots 0 .. W-1.
//   4. thread 0 commits the step: (token, parent) into trace, r = lp, the next step's tokens, sum = p.  s_q stays valid for the
//      caller, whose threads gather slot v's state from parent s_q[v].
//   5. still thread 0, for v = 0 .. W-1 in order: a token 0, or t = L-1, enters the video's best-W done list with score p, AFTER
//      entries of equal score (so the list is the first W of a stable descending sort of every completion), and sum[v] = -1000.
//      With a `scale` table in the book (include/xgate_beam_rules.h) the list is ordered by KEY instead: key = p * scale[t] (one
//      fp32 multiply) for a live p > -500, else p; done_key holds the keys beside done_score.  scale == null: the rule above.
// beam_backtrace_row then follows a done entry's parents back through trace.
// Plain stores from one lane, no atomics, one fixed order for every sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/xgate_beam.h"
#include "../../include/xgate_pos_beam.h"

static_assert(XGCB_MAX_BEAM == XGPB_MAX_BEAM, "both searches share BeamTables and beam_merge");
constexpr int XG_BEAM_MAX = XGCB_MAX_BEAM;
static_assert(XG_BEAM_MAX * XG_BEAM_MAX <= 64, "one wave ranks a video's candidates");

// the bookkeeping of a search.  Tok: int64_t for the captioner (core_step reads int64 tokens), int32_t for the POS generator
template <typename Tok>
struct BeamBook {
    float* sum;                  // (M) running sums (not read at t = 0)
    Tok* tok;                    // (M) the step's tokens, fed by the next step
    int32_t* trace;              // (B,L,W,2) (token, parent) of every slot and step
    float* r;                    // (B,L,W) the log-probability of that token
    int32_t* trace_out;          // the caller's copy of trace, or null
    float* done_score;           // (B,W) the best completions so far, descending
    int32_t* done_at;            // (B,W,2) their (step, slot)
    int32_t* done_n;             // (B) how many (not read at t = 0)
    int L, W, t;
    const float* scale;          // (L) the done list's length scale, or null: the list is ordered by score
    float* done_key;             // (B,W) the keys of the done list; only with `scale`
};

// the book's regions out of a workspace, in their one order; trace_out and t are the call's.  Carver: take<T>(n)
template <typename Tok, typename Carver>
inline BeamBook<Tok> beam_book_carve(Carver& c, size_t B, size_t W, size_t L) {
    BeamBook<Tok> k{};
    const size_t M = B * W;
    k.sum = c.template take<float>(M); k.tok = c.template take<Tok>(M);
    k.trace = c.template take<int32_t>(B * L * W * 2); k.r = c.template take<float>(B * L * W);
    k.done_score = c.template take<float>(M); k.done_at = c.template take<int32_t>(M * 2); k.done_n = c.template take<int32_t>(B);
    k.L = (int)L; k.W = (int)W;
    return k;
}

// a merge workgroup's LDS tables: the candidates [q * XG_BEAM_MAX + k] (c_p: [candidate]) and the new slots [v]
struct BeamTables {
    float c_lp[XG_BEAM_MAX * XG_BEAM_MAX], c_p[XG_BEAM_MAX * XG_BEAM_MAX];
    int c_tok[XG_BEAM_MAX * XG_BEAM_MAX];
    float s_lp[XG_BEAM_MAX], s_p[XG_BEAM_MAX];
    int s_q[XG_BEAM_MAX], s_tok[XG_BEAM_MAX];
};
static_assert(sizeof(BeamTables) == 896, "the fixed part of XGPB_LDS_BYTES (1024) accounts for 896 bytes of tables");

constexpr float XG_BEAM_LIVE = -500.0f;      // the dead-slot rule: a sum at or below this carries a -1000

// the order of the search: is (v, i) before (ov, oi)?  Larger value first, lower index first on exact ties.  Total on non-NaN
// values; a NaN is before nothing and nothing is before it, so it ranks nowhere and is never kept.
__device__ __forceinline__ bool beam_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// steps 3-5 for video b, called by ALL threads of the workgroup (>= 64) once c_lp / c_tok are written (no barrier needed before)
template <typename Tok>
__device__ __forceinline__ void beam_merge(BeamTables& T, const BeamBook<Tok>& k, size_t b, int rows) {
    const int tid = threadIdx.x, W = k.W, t = k.t, L = k.L;
    const size_t row0 = b * W;
    // (a NaN ranks nowhere: whatever stays unwritten below is slot 0 / token 0, never an index out of range)
    if (tid < XG_BEAM_MAX) { T.s_lp[tid] = 0.f; T.s_p[tid] = 0.f; T.s_q[tid] = 0; T.s_tok[tid] = 0; }
    __syncthreads();
    const int ncand = W * rows;               // candidate i = c_rank * rows + q
    int cq = 0, cr = 0;
    float p = 0.f;
    if (tid < ncand) {
        cr = tid / rows;
        cq = tid - cr * rows;
        p = (t == 0 ? 0.f : k.sum[row0 + cq]) + T.c_lp[cq * XG_BEAM_MAX + cr];
        T.c_p[tid] = p;
    }
    __syncthreads();
    if (tid < ncand) {                        // stable descending rank; the first W are the new slots
        int rank = 0;
        for (int i = 0; i < ncand; ++i) rank += beam_before(T.c_p[i], i, p, tid) ? 1 : 0;
        if (rank < W) {
            T.s_q[rank] = cq;
            T.s_tok[rank] = T.c_tok[cq * XG_BEAM_MAX + cr];
            T.s_lp[rank] = T.c_lp[cq * XG_BEAM_MAX + cr];
            T.s_p[rank] = p;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    float* ds = k.done_score + row0;
    float* dk = k.scale ? k.done_key + row0 : ds;             // what the list is ordered by
    int32_t* da = k.done_at + row0 * 2;
    int n = t == 0 ? 0 : k.done_n[b];
    n = n < 0 ? 0 : (n > W ? W : n);
    for (int v = 0; v < W; ++v) {
        const size_t e = (b * L + t) * W + v;
        k.trace[2 * e] = T.s_tok[v];
        k.trace[2 * e + 1] = T.s_q[v];
        if (k.trace_out) { k.trace_out[2 * e] = T.s_tok[v]; k.trace_out[2 * e + 1] = T.s_q[v]; }
        k.r[e] = T.s_lp[v];
        k.tok[row0 + v] = T.s_tok[v];
        float sm = T.s_p[v];
        if (T.s_tok[v] == 0 || t == L - 1) {
            float key = sm;
            if (k.scale && sm > XG_BEAM_LIVE) key = __fmul_rn(sm, k.scale[t]);
            int pos = n;
            while (pos > 0 && dk[pos - 1] < key) --pos;        // after entries of equal score (key)
            if (pos < W) {
                const int last = n < W ? n : W - 1;
                for (int i = last; i > pos; --i) {
                    ds[i] = ds[i - 1]; da[2 * i] = da[2 * i - 2]; da[2 * i + 1] = da[2 * i - 1];
                    if (k.scale) dk[i] = dk[i - 1];
                }
                ds[pos] = sm; da[2 * pos] = t; da[2 * pos + 1] = v;
                if (k.scale) dk[pos] = key;
                if (n < W) ++n;
            }
            sm = -1000.0f;
        }
        k.sum[row0 + v] = sm;
    }
    k.done_n[b] = n;
}

// done entry i = (video, rank): its score, and its beam read back along its parents into seq / seq_logp (M,L), zero after its
// finish
template <typename Tok>
__device__ __forceinline__ void beam_backtrace_row(const BeamBook<Tok>& k, size_t i, int64_t* seq, float* seq_logp, float* score) {
    const int W = k.W, L = k.L;
    const size_t b = i / W;
    int tf = k.done_at[2 * i], s = k.done_at[2 * i + 1];
    tf = tf < 0 ? 0 : (tf >= L ? L - 1 : tf);
    int64_t* sq = seq + i * L;
    float* lp = seq_logp + i * L;
    score[i] = k.done_score[i];
    for (int t = L - 1; t > tf; --t) { sq[t] = 0; lp[t] = 0.f; }
    for (int t = tf; t >= 0; --t) {
        s = s < 0 ? 0 : (s >= W ? W - 1 : s);
        const size_t e = (b * L + t) * W + s;
        sq[t] = k.trace[2 * e];
        lp[t] = k.r[e];
        s = k.trace[2 * e + 1];
    }
}

// ---- The group form (diverse beam search, include/xgate_beam_diverse.h and include/xgate_pos_beam_diverse.h).  A pair (one "video" of
// the plain rule) owns N = Gd * Wg slots, group j the slots j Wg .. (j + 1) Wg - 1; each group is a search of width Wg by the rule
// above with its own sums, done list and ranking, so the book is carved as (pairs * Gd, Wg, L) and beam_backtrace_row serves it
// unchanged.  Within a step the groups of a pair are merged in series, j = 0 .. Gd-1, by ONE workgroup:
//   a. beam_group_rerank (one wave per row of the group): the value selected by is a = lp - lambda * n_j(token), n_j = how many
//      LIVE (new sum p > -500) new slots of groups 0 .. j-1 took that token at this step; (float)n * lambda and the subtraction are
//      rounded each on its own (never an FMA).  The row's Wg best a, lower token first on exact ties, enter the candidate tables
//      with the unpenalised lp beside them.
//   b. beam_group_merge (all threads): steps 3-5 over a; sum = p carries the penalties, r is the UNPENALISED lp, the parents of the
//      pair go to G.par (pair slot indices) for the caller's state gather, the caller's trace is (pairs,L,N,2) with pair slot
//      parents, and the group's live new tokens join the penalty list.  Ends with a barrier: the next group may start at once.
// n_j(v) = 0 or lambda = 0 leave lp as it is (lp - 0), so Gd = 1 is beam_merge bit for bit.
struct BeamGroupTables {
    BeamTables T;
    float c_r[XG_BEAM_MAX * XG_BEAM_MAX];    // the unpenalised lp of candidate entry [q * XG_BEAM_MAX + k]
    int par[XG_BEAM_MAX];                    // the pair's parents, as pair slot indices
    int pen_tok[XG_BEAM_MAX];                // tokens of the earlier groups' live new slots, one entry per slot
    int pen_n;
};

// all threads, once per pair and step, before group 0 (no barrier needed before the first rerank's own)
__device__ __forceinline__ void beam_group_begin(BeamGroupTables& G) {
    const int tid = threadIdx.x;
    if (tid < XG_BEAM_MAX * XG_BEAM_MAX) { G.T.c_lp[tid] = 0.f; G.T.c_tok[tid] = 0; G.c_r[tid] = 0.f; }
    if (tid < XG_BEAM_MAX) { G.par[tid] = 0; G.pen_tok[tid] = 0; }
    if (tid == 0) G.pen_n = 0;
    __syncthreads();
}

// a = lp - lambda * n(tok): one multiply and one subtraction, each rounded on its own
__device__ __forceinline__ float beam_penalised(const BeamGroupTables& G, float lp, int tok, float lambda) {
    int n = 0;
    for (int i = 0; i < G.pen_n; ++i) n += G.pen_tok[i] == tok ? 1 : 0;
    return __fsub_rn(lp, __fmul_rn((float)n, lambda));
}

// one wave (lane = 0 .. 63) for row q of the group: entries e < ne are (lp[e], tok ? tok[e] clamped to [0, tok_max] : e), DISTINCT
// tokens; the Wg best penalised values, lower token first on exact ties, into the tables of row q.  Needs ne >= Wg.
__device__ __forceinline__ void beam_group_rerank(BeamGroupTables& G, int q, const float* lp, const int32_t* tok, int ne, int tok_max,
                                                  int Wg, float lambda, int lane) {
    auto token = [&](int e) { const int v = tok ? tok[e] : e; return v < 0 ? 0 : (v > tok_max ? tok_max : v); };
    for (int e = lane; e < ne; e += 64) {
        const int tk = token(e);
        const float r = lp[e], a = beam_penalised(G, r, tk, lambda);
        int rank = 0;
        for (int f = 0; f < ne && rank < Wg; ++f) {
            const int tf = token(f);
            rank += beam_before(beam_penalised(G, lp[f], tf, lambda), tf, a, tk) ? 1 : 0;
        }
        if (rank < Wg) { G.T.c_lp[q * XG_BEAM_MAX + rank] = a; G.T.c_tok[q * XG_BEAM_MAX + rank] = tk; G.c_r[q * XG_BEAM_MAX + rank] = r; }
    }
}

// steps 3-5 for group j of pair `pair`, called by ALL threads of the workgroup (>= 64) after a barrier behind the reranks of the
// group's rows.  k: the book carved as (pairs * Gd, Wg, L), k.W = Wg; trace_out (pairs,L,Gd*Wg,2) or null.
template <typename Tok>
__device__ __forceinline__ void beam_group_merge(BeamGroupTables& G, const BeamBook<Tok>& k, size_t pair, int Gd, int j, int rows) {
    BeamTables& T = G.T;
    const int tid = threadIdx.x, W = k.W, t = k.t, L = k.L, N = Gd * W;
    const size_t g = pair * Gd + j, row0 = g * W;
    if (tid < XG_BEAM_MAX) { T.s_lp[tid] = 0.f; T.s_p[tid] = 0.f; T.s_q[tid] = 0; T.s_tok[tid] = 0; }
    __syncthreads();
    const int ncand = W * rows;               // candidate i = c_rank * rows + q
    int cq = 0, cr = 0;
    float p = 0.f;
    if (tid < ncand) {
        cr = tid / rows;
        cq = tid - cr * rows;
        p = (t == 0 ? 0.f : k.sum[row0 + cq]) + T.c_lp[cq * XG_BEAM_MAX + cr];
        T.c_p[tid] = p;
    }
    __syncthreads();
    if (tid < ncand) {                        // stable descending rank; the first W are the new slots.  s_lp: the unpenalised lp
        int rank = 0;
        for (int i = 0; i < ncand; ++i) rank += beam_before(T.c_p[i], i, p, tid) ? 1 : 0;
        if (rank < W) {
            T.s_q[rank] = cq;
            T.s_tok[rank] = T.c_tok[cq * XG_BEAM_MAX + cr];
            T.s_lp[rank] = G.c_r[cq * XG_BEAM_MAX + cr];
            T.s_p[rank] = p;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float* ds = k.done_score + row0;
        int32_t* da = k.done_at + row0 * 2;
        int n = t == 0 ? 0 : k.done_n[g];
        n = n < 0 ? 0 : (n > W ? W : n);
        int pn = G.pen_n;
        for (int v = 0; v < W; ++v) {
            const size_t e = (g * L + t) * W + v;
            k.trace[2 * e] = T.s_tok[v];
            k.trace[2 * e + 1] = T.s_q[v];
            G.par[j * W + v] = j * W + T.s_q[v];
            if (k.trace_out) {
                const size_t eo = (pair * L + t) * N + (size_t)j * W + v;
                k.trace_out[2 * eo] = T.s_tok[v];
                k.trace_out[2 * eo + 1] = j * W + T.s_q[v];
            }
            k.r[e] = T.s_lp[v];
            k.tok[row0 + v] = T.s_tok[v];
            float sm = T.s_p[v];
            if (sm > XG_BEAM_LIVE && pn < XG_BEAM_MAX) G.pen_tok[pn++] = T.s_tok[v];      // (token 0 counts like any other)
            if (T.s_tok[v] == 0 || t == L - 1) {
                int pos = n;
                while (pos > 0 && ds[pos - 1] < sm) --pos;         // after entries of equal score
                if (pos < W) {
                    const int last = n < W ? n : W - 1;
                    for (int i = last; i > pos; --i) { ds[i] = ds[i - 1]; da[2 * i] = da[2 * i - 2]; da[2 * i + 1] = da[2 * i - 1]; }
                    ds[pos] = sm; da[2 * pos] = t; da[2 * pos + 1] = v;
                    if (n < W) ++n;
                }
                sm = -1000.0f;
            }
            k.sum[row0 + v] = sm;
        }
        k.done_n[g] = n;
        G.pen_n = pn;
    }
    __syncthreads();
}
