/*
 * xgate_beam_control.h -- C ABI of the CAPTIONER'S BEAM SEARCH UNDER S POS TEMPLATES PER VIDEO in libxgate_hip.so (gfx950): the W
 * most likely captions of each of B videos under each of its S `pos_feats` rows, on one shared encoder pass.  It is the
 * beam search of xgate_beam.h on the batch in which every video is repeated S times, without the repeat.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h, xgate_beam.h and xgate_control.h: device pointers, caller-owned memory,
 * every entry point only ENQUEUES work on `stream`, arguments are checked before anything is enqueued, and a call does not depend
 * on what the workspace held before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1.  A GROUP is one (video b, template s)
 * pair, g = b * S + s, G = B * S groups; one row is one (group, slot) pair with row index (b * S + s) * W + slot.  The encoder,
 * init_hidden and v2a(V) run once on the B videos and are NOT row-repeated: only the initial state (4 B S W R floats) and
 * pos_feats (B S W R) are.  The attention of a step reads a video's v2a(V) and V once for every attention group (xgate_control.h) of its
 * S W rows; no step needs the host.
 */
#ifndef XGATE_BEAM_CONTROL_H
#define XGATE_BEAM_CONTROL_H

#include "xgate_beam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGBC_VERSION 1

int xgbc_version(void);
/* bytes of the workspace of xgbc_beam_search at dims d (d->B = VIDEOS) with S templates per video and beam width W: the per-video
 * encoder part, the (B S W)-row step part -- what the workspace of xgate_beam.h's search holds less the row-repeated (M,K,R) and (M,K,A) blocks -- and
 * the search tables of the B S groups in one block; 0 for whatever that call refuses with XG_EINVAL on account of d, S and W */
size_t xgbc_workspace_bytes(const XgDims *d, int32_t S, int32_t W);

/*
 * Beam search per group.  Every group runs the search of xgate_beam.h on its own: W slots with running sums sum[W] = 0, all
 * starting from its VIDEO's init_hidden state, all gated by the group's pos_feats row.  For t = 0 .. L-1:
 *   1. the decoder step on every slot with mask 1, fed BOS (0) at t = 0 and the slot's token of step t - 1 after it.  Dead slots
 *      keep running.
 *   2. lp[q][v] = log_softmax(logit(h2_q))[v], then lp[q][suppress_token] -= 1000 when suppress_token >= 0 (any negative value
 *      turns it off).
 *   3. rows = 1 at t = 0, else W.  Per row the W largest lp in descending order, lower word index first on exact ties of the fp32
 *      lp; candidate c_rank * rows + q has p = sum[q] + lp (one fp32 add); a stable sort by p descending; the first W are the new
 *      slots 0 .. W-1.
 *   4. new slot v takes the whole state (h1, c1, h2, c2) of its parent slot q; its token is the candidate's word,
 *      r[t][v] = lp (the -1000 included), sum[v] = p.
 *   5. for v = 0 .. W-1 in order: a token 0, or t = L-1, appends the beam to the group's done list with score p and sets
 *      sum[v] = -1000.  The done beam holds its tokens and r for steps 0 .. t, zeros after.
 * The result per group is its done list stable-sorted by score descending, first W entries (at least W always exist): each beam
 * is ranked by its score AT THE MOMENT IT FINISHED.  Groups never interact: a group's result depends on its video and its
 * pos_feats row, not on s or on the other templates.
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (B*S,R), row
 *                         b * S + s; seq / seq_mask are not read
 *   seq (G,W,L)           int64 out: a done beam's tokens, zero after its finish
 *   seq_logp (G,W,L)      its r, zero after its finish
 *   score (G,W)           its p
 *   trace (G,L,W,2)       int32 (token, parent slot) of every slot and step; NULL: not stored
 * XG_EINVAL, before anything is enqueued: everything the search of xgate_beam.h refuses (W < 1, W > V, W above its widest beam, 8,
 * suppress_token >= V, run->train, run->save, a run->gemm_mode other than 0, a null pointer other than `trace` -- bn and its four
 * statistics included --, invalid dims, d->T < 2 among them, a workspace that is not 256-byte aligned), S < 1, and B * S * W beyond
 * 2^20 rows.  XG_EWORKSPACE: ws_bytes below xgbc_workspace_bytes(d, S, W).
 */
int xgbc_beam_search(void *stream, const XgDims *d, int32_t S, int32_t W, int32_t suppress_token, const XgParams *p,
                     const XgBnState *bn, const XgBatch *x, const XgRun *run, int64_t *seq, float *seq_logp, float *score,
                     int32_t *trace, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_BEAM_CONTROL_H */
