/*
 * xgate_pos_beam.h -- C ABI of POS BEAM SEARCH in libxgate_hip.so (gfx950): the W most likely templates the generator itself gives
 * each of B videos, the search of pos_src/SAModel.py:104-134 and pos_src/CaptionModel.py:22-125.  What it writes to `templates` is
 * directly a valid input of xgpc_sample_forced (xgate_pos_control.h).
 *
 * Eval mode, fp32.  The conventions are those of xgate_pos_control.h: device pointers, caller-owned memory, d->B counts VIDEOS,
 * d->T = seq_length + 1 = L + 1, one row is one (video b, slot) pair with row index b * W + slot, every entry point only ENQUEUES
 * work on `stream`, arguments are checked before anything is enqueued, and a call does not depend on what the workspace held
 * before.  No step needs the host: a video's whole merge (W rows of C log-probabilities, W * W candidates) runs in one workgroup.
 */
#ifndef XGATE_POS_BEAM_H
#define XGATE_POS_BEAM_H

#include "xgate_pos_control.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPB_VERSION 1

/* the widest beam: W * W <= 64 candidates are ranked by one wave */
#define XGPB_MAX_BEAM 8

/* LDS bytes of a video's merge workgroup: h and c of its W rows, their W x C logits, and 1024 bytes of fixed tables.  A call
 * whose dims need more than the 64 KiB a workgroup gets without opting in is refused (W = 8 holds up to R = 998 at C = 20). */
#define XGPB_LDS_BYTES(W, R, C) (4 * (size_t)(W) * (2 * (size_t)(R) + (size_t)(C)) + 1024)
#define XGPB_MAX_LDS_BYTES 65536

int xgpb_version(void);
/* bytes of the workspace of xgpb_beam_templates at dims d with beam width W; 0 for whatever that call refuses with XG_EINVAL on
 * account of d and W */
size_t xgpb_workspace_bytes(const XgpDims *d, int32_t W);

/*
 * Beam search.  Per video W slots with running sums sum[W] = 0, all starting from the video's init_hidden state.  For t = 0 .. L-1:
 *   1. the cell on every slot with mask 1, fed BOS (0) at t = 0 and the slot's token of step t - 1 after it.  Dead slots keep
 *      running (there is no hold).
 *   2. lp[q][c] = log_softmax(logit(h_q))[c], then lp[q][suppress_tag] -= 1000 when suppress_tag >= 0 (the reference does this for
 *      category 1, CaptionModel.py:92; any negative value turns it off).
 *   3. rows = 1 at t = 0, else W.  Per row the W largest lp in descending order, lower category first on exact ties; candidate
 *      c_rank * rows + q has p = sum[q] + lp (one fp32 add); a stable sort by p descending; the first W are the new slots 0 .. W-1.
 *   4. new slot v takes h and c of its parent slot q; its token is c, r[t][v] = lp (the -1000 included), sum[v] = p.
 *   5. for v = 0 .. W-1 in order: a token 0, or t = L-1, appends the beam to the video's done list with score p and sets
 *      sum[v] = -1000.  The done beam holds its tokens and r for steps 0 .. t, zeros after.
 * The result per video is its done list stable-sorted by score descending, first W entries (at least W always exist): each beam
 * is ranked by its score AT THE MOMENT IT FINISHED.
 *   templates (B,W,L)     int64 out: a done beam's tokens, zero after its finish
 *   tag_logp (B,W,L)      its r, zero after its finish (the end tag counts, as in the forced call)
 *   score (B,W)           its p
 *   masks (B,W,L+1)       column 0 is 1, column t is 1 while the first t tokens are all non-zero (the forced call's mask)
 *   n_out (device int32[1]) from masks as in xgpc_sample_forced; 0 is legal
 *   trace (B,L,W,2)       int32 (token, parent slot) of every slot and step; NULL: not stored
 * XG_EINVAL, before anything is enqueued: W < 1, W > C (the reference asserts this), W > XGPB_MAX_BEAM, suppress_tag >= C,
 * XGPB_LDS_BYTES(W, R, C) > XGPB_MAX_LDS_BYTES, a null pointer other than `trace`, invalid dims (those of xgpc_sample_forced at
 * S = W).  XG_EWORKSPACE: ws_bytes below xgpb_workspace_bytes(d, W).
 */
int xgpb_beam_templates(void *stream, const XgpDims *d, int32_t W, int32_t suppress_tag, const XgpParams *p, const XgBnState *bn,
                        const float *feats_rgb, const float *feats_opfl, const float *feat_mask, int64_t *templates,
                        float *tag_logp, float *score, float *masks, int32_t *n_out, int32_t *trace, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_BEAM_H */
