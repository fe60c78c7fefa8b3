/*
 * xgate_ss.h -- C ABI of the FUSED TEACHER-FORCED LOSS UNDER SCHEDULED SAMPLING in libxgate_hip.so (gfx950): the loss of
 * xg_xe_loss_fwd / xg_xe_loss_bwd (xgate.h) and of its form with Q captions per video (xgate_train_video.h) with the token that
 * feeds a step drawn, where a coin says so, from the step before (caption_src/SAModel.py:89-99).  What SAModel.xe_loss_ss and
 * SAModel.xe_loss_ss_per_video run.  No (rows, T, V) log-probability tensor and no gradient of one is formed.
 *
 * fp32 data path (XgRun.gemm_mode 0).  The conventions are those of xgate.h: device pointers, caller-owned memory, the entry points
 * only ENQUEUE work on `stream`, arguments are checked before anything is enqueued, every output element is written, and no call
 * depends on what the workspace held before the forward.
 *
 * Q == 0, the plain form: d->B rows, x as xg_xe_loss_fwd takes it, M = B.
 * Q >= 1, the per-video form: d->B counts VIDEOS, x as the per-video loss of xgate_train_video.h takes it (the videos once;
 *         pos_feats (M,R), seq (M,T), seq_mask (M,T), cap_classes and class_mask per row), row b * Q + q is caption q of video b,
 *         M = B Q.
 *
 * Steps t = 0 .. T-1, T = d->T.  In train mode with ss_prob > 0, row m of step t >= 1 is fed a drawn token iff
 * u_sel[t * M + m] < ss_prob (strict); every other row, and every row of step 0, is fed seq[m, t].  The drawn token is the first
 * index whose running sum of exp(logit_v - max) over step t - 1's logits exceeds u_tok[t * M + m] times the total: inverse CDF at
 * temperature 1.  u_sel and u_tok are (T, M) float32; row 0 of either is not read.  The loss is that of xg_xe_loss_fwd over the
 * logits this token stream produces, against seq and seq_mask; the state update keeps using seq_mask[:, t] and all T steps run.
 * No gradient flows through the choice: the backward is that of the teacher-forced loss with the fed tokens in place of seq on
 * the token side and in the embedding scatter.  BatchNorm and dropout are those of the teacher-forced entry point of the same form.
 * Eval mode or ss_prob == 0: nothing is drawn and tok_out holds seq, time-major.
 */
#ifndef XGATE_SS_H
#define XGATE_SS_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGSS_VERSION 1

int xgss_version(void);
/* bytes of the workspace.  Q == 0: xg_workspace_bytes_mode(d, 0) -- the plain form runs in a standard fp32 workspace.  Q >= 1: the
 * per-video part and the (B Q)-row part of the per-video loss's workspace (xgate_train_video.h) plus the fed tokens and the tile
 * statistics of a step.  0 for invalid dims, Q < 0, or more than 2^20 rows. */
size_t xgss_workspace_bytes(const XgDims *d, int32_t Q);

/*
 * losses[0..2] (device) = total, language-model and classifier loss, as xg_xe_loss_fwd leaves them; tok_out (T, M) int64 (device)
 * = the fed tokens.  cap_classes == NULL: no classifier term.  The workspace afterwards holds what xgss_xe_loss_bwd needs.
 * XG_EINVAL, before anything is enqueued: invalid dims, Q < 0, more than 2^20 rows or a null workspace; then, behind the size
 * test below: a workspace that is not 256-byte aligned, a null pointer (p, x and its six fields, run, losses, tok_out; u_sel and
 * u_tok when run->train and ss_prob > 0; in eval mode bn and its four statistics), ss_prob outside [0, 1], a run->gemm_mode other
 * than 0.
 * XG_EWORKSPACE: ws_bytes below xgss_workspace_bytes(d, Q).
 */
int xgss_xe_loss_fwd(void *stream, const XgDims *d, int32_t Q, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                     const int64_t *cap_classes, const float *class_mask, float weight_class, float ss_prob, const float *u_sel,
                     const float *u_tok, const XgRun *run, void *ws, size_t ws_bytes, float *losses, int64_t *tok_out);
/*
 * g += dloss_dev[0] * d(losses[0]) / d(parameter) for every parameter, from the workspace xgss_xe_loss_fwd left, with the same
 * d, Q, x, cap_classes, class_mask, weight_class and run (run->grad_event / grad_event_head as in xg_xe_loss_bwd).  The gates are
 * those of the forward (g and dloss_dev among the pointers; no uniforms, no outputs).
 */
int xgss_xe_loss_bwd(void *stream, const XgDims *d, int32_t Q, const XgParams *p, const XgParams *g, const XgBatch *x,
                     const int64_t *cap_classes, const float *class_mask, float weight_class, const float *dloss_dev,
                     const XgRun *run, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_SS_H */
