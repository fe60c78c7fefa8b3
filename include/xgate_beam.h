/*
 * xgate_beam.h -- C ABI of the CAPTIONER'S BEAM SEARCH in libxgate_hip.so (gfx950): the W most likely captions of each of B videos,
 * the search of caption_src/SAModel.py:129-161 and caption_src/CaptionModel.py:22-128 (what controllable_xgating_amd/beam.py runs
 * with one host round trip per step), as one enqueue.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h: device pointers, caller-owned memory, every entry point only ENQUEUES
 * work on `stream`, arguments are checked before anything is enqueued, and a call does not depend on what the workspace held
 * before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1, one row is one (video b, slot) pair with row index b * W + slot.
 * The encoder, init_hidden and v2a(V) run once on the B videos and are row-repeated on the device; no step needs the host.
 */
#ifndef XGATE_BEAM_H
#define XGATE_BEAM_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGCB_VERSION 1

/* the widest beam: W * W <= 64 candidates are ranked by one wave */
#define XGCB_MAX_BEAM 8

int xgcb_version(void);
/* bytes of the workspace of xgcb_beam_search at dims d with beam width W: the per-video encoder part, the (B W)-row step part
 * and the search tables in one block; 0 for whatever that call refuses with XG_EINVAL on account of d and W */
size_t xgcb_workspace_bytes(const XgDims *d, int32_t W);

/*
 * Beam search.  Per video W slots with running sums sum[W] = 0, all starting from the video's init_hidden state.  For t = 0 .. L-1:
 *   1. the decoder step on every slot with mask 1, fed BOS (0) at t = 0 and the slot's token of step t - 1 after it.  Dead slots
 *      keep running.
 *   2. lp[q][v] = log_softmax(logit(h2_q))[v], then lp[q][suppress_token] -= 1000 when suppress_token >= 0 (the reference does
 *      this for UNK, index 1, CaptionModel.py:94; any negative value turns it off).
 *   3. rows = 1 at t = 0, else W.  Per row the W largest lp in descending order, lower word index first on exact ties of the fp32
 *      lp; candidate c_rank * rows + q has p = sum[q] + lp (one fp32 add); a stable sort by p descending; the first W are the new
 *      slots 0 .. W-1.
 *   4. new slot v takes the whole state (h1, c1, h2, c2) of its parent slot q; its token is the candidate's word,
 *      r[t][v] = lp (the -1000 included), sum[v] = p.
 *   5. for v = 0 .. W-1 in order: a token 0, or t = L-1, appends the beam to the video's done list with score p and sets
 *      sum[v] = -1000.  The done beam holds its tokens and r for steps 0 .. t, zeros after.
 * The result per video is its done list stable-sorted by score descending, first W entries (at least W always exist): each beam
 * is ranked by its score AT THE MOMENT IT FINISHED.
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K), pos_feats (B,R); seq / seq_mask are not read
 *   seq (B,W,L)           int64 out: a done beam's tokens, zero after its finish
 *   seq_logp (B,W,L)      its r, zero after its finish
 *   score (B,W)           its p
 *   trace (B,L,W,2)       int32 (token, parent slot) of every slot and step; NULL: not stored
 * XG_EINVAL, before anything is enqueued: W < 1, W > V, W > XGCB_MAX_BEAM, suppress_token >= V, run->train, run->save, a
 * run->gemm_mode other than 0, a null pointer other than `trace` (bn and its four statistics included: eval mode reads them),
 * invalid dims (d->T < 2 among them), a workspace that is not 256-byte aligned.  XG_EWORKSPACE: ws_bytes below
 * xgcb_workspace_bytes(d, W).
 */
int xgcb_beam_search(void *stream, const XgDims *d, int32_t W, int32_t suppress_token, const XgParams *p, const XgBnState *bn,
                     const XgBatch *x, const XgRun *run, int64_t *seq, float *seq_logp, float *score, int32_t *trace, void *ws,
                     size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_BEAM_H */
