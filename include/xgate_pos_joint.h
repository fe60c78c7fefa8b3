/*
 * xgate_pos_joint.h -- C ABI of the POS sequence generator's side of JOINT TRAINING in libxgate_hip.so (gfx950): the state the
 * captioner consumes as an output of the train-mode forward, and its gradient as an input of the backward
 * (docs/JOINT_TRAINING.md).  What PosModel.forward(..., return_pos_feats=True) runs.
 *
 * The conventions, XgptRun and the workspace are those of xgate_pos_train.h; nothing here changes its entry points.
 */
#ifndef XGATE_POS_JOINT_H
#define XGATE_POS_JOINT_H

#include "xgate_pos_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPJ_VERSION 1

int xgpj_version(void);

/*
 * pos_feats (B,R) = the state behind step Tp - 1 of the last xgpt_forward_train on ws (1 <= Tp <= d->T; Tp = the forward's
 * t_out is the state the reference's loop ends with, caption_src/data_io.py:215-216 reads states[-1]).  With train-mode dropout it
 * is the state AFTER the site-6 mask, held rows included: what the loop carries into the next step.
 * XG_EINVAL, before anything is enqueued: invalid dims, Tp outside [1, d->T], a null ws or pos_feats; XG_EWORKSPACE: ws_bytes below
 * xgpt_workspace_bytes(d).
 */
int xgpj_final_state(void *stream, const XgpDims *d, int32_t Tp, const void *ws, size_t ws_bytes, float *pos_feats);

/*
 * xgpt_backward with the gradient of the loss with respect to xgpj_final_state(Tp)'s result as one more input: the reverse-time
 * loop's first dH is dpos (B,R) instead of zero.  dlogp == NULL means all zero (a gradient through pos_feats alone): no
 * (B,Tp,C) buffer is read, and logit.weight / logit.bias receive exactly zero.  dpos == NULL means all zero: xgpt_backward.  Both
 * NULL: XG_EINVAL.  Everything else as xgpt_backward (same gates, gradients ADDED into g).
 */
int xgpj_backward(void *stream, const XgpDims *d, const XgpParams *p, const XgpParams *g, const XgptRun *run,
                  const float *feats_rgb, const float *feats_opfl, const float *feat_mask, int32_t Tp,
                  const float *dlogp, void *ws, size_t ws_bytes, const float *dpos);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_JOINT_H */
