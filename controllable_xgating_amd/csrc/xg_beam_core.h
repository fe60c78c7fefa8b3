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
