/*
 * xgate_joint.h -- C ABI of the CAPTION LOSS'S GRADIENT WITH RESPECT TO pos_feats in libxgate_hip.so (gfx950): what joint training
 * of the captioner and the POS sequence generator sends from the first into the second (docs/JOINT_TRAINING.md).  What
 * SAModel.xe_loss, xe_loss_per_video, xe_loss_ss and xe_loss_ss_per_video run behind their backward when pos_feats requires a
 * gradient, and only then.
 *
 * The conventions are those of xgate.h: device pointers, caller-owned memory, the entry point only ENQUEUES work on `stream`, and
 * arguments are checked before anything is enqueued.
 *
 * Every fused-loss backward leaves, for each of its T = d->T steps, the gradient of the loss with respect to the gated POS vector
 * (DPOSG, (T,M,R)) next to the gate values the forward kept (GP, (T,M,R), after the gate's dropout); dloss_dev is folded into
 * DPOSG.  The gate is y = g * pos + pos (sub_modules.py:45), so
 *
 *     dpos[m, j] = sum over t = 0 .. T-1 of  DPOSG[t, m, j] * (GP[t, m, j] + 1)
 *
 * The backward visits all T steps whatever the captions' lengths are (its reverse-time loop has no early stop, and the
 * products that fill DPOSG cover the step ranges [0, T) between them with plain stores), so the sum runs over all T rows and every
 * one of them has been written by the backward that precedes the call.
 */
#ifndef XGATE_JOINT_H
#define XGATE_JOINT_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGJ_VERSION 1

/* which backward left the workspace, i.e. its layout */
#define XGJ_FORM_XE 0        /* xg_xe_loss_bwd (xgate.h): Q == 0, M = d->B rows */
#define XGJ_FORM_VIDEO 1     /* the per-video loss's backward (xgate_train_video.h): Q >= 1, M = d->B * Q rows */
#define XGJ_FORM_SS 2        /* the scheduled-sampling loss's backward (xgate_ss.h): Q == 0 or Q >= 1 */

int xgj_version(void);

/*
 * Behind the fused-loss backward of `form` on the same stream and workspace, with the same d and Q: dpos (M,R), row b * Q + q in
 * the per-video forms, is WRITTEN (plain stores, every element).  One writer per element, the T terms added in step order, no
 * float atomics: the same call gives the same bits.  x and run are those of the backward (neither is read: the sum needs only the
 * workspace).
 * XG_EINVAL, before anything is enqueued: invalid dims, a null pointer (x, run, ws, dpos), an unknown form, a Q that does not fit
 * the form, too many rows for the form, a workspace that is not 256-byte aligned, or ws_bytes below the form's workspace size
 * (xg_workspace_bytes_mode(d, 0), or what the workspace_bytes function of xgate_train_video.h / xgate_ss.h returns for d and Q).
 */
int xgj_caption_dpos(void *stream, const XgDims *d, int32_t Q, int32_t form, const XgBatch *x, const XgRun *run, void *ws,
                     size_t ws_bytes, float *dpos);

/* For tests and tools: 4 when the last xgj_caption_dpos of this process ran its four-wide kernel, 1 for the scalar one, 0 before
 * the first call.  The choice: R % 4 == 0 and 16-byte aligned DPOSG, GP and dpos, as the gate's backward decides for its kernel. */
int xgj_last_kernel_width(void);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_JOINT_H */
