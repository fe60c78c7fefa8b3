/*
 * xgate_train_video.h -- C ABI of TEACHER-FORCED TRAINING ON Q CAPTIONS PER VIDEO in libxgate_hip.so (gfx950): the fused
 * cross-entropy loss of xg_xe_loss_fwd / xg_xe_loss_bwd (xgate.h) with the B videos handed over ONCE and Q caption rows each.
 * What SAModel.xe_loss_per_video runs.
 *
 * fp32 data path (XgRun.gemm_mode 0), train and eval mode.  The conventions are those of xgate.h: device pointers, caller-owned
 * memory, the entry points only ENQUEUE work on `stream`, arguments are checked before anything is enqueued, and no call depends
 * on what the workspace held before the forward.  d->B counts VIDEOS, d->T = seq_length + 1.  Row b * Q + q is caption q of video
 * b; M = B Q rows.
 *
 *   x   feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE;
 *       pos_feats (M,R), seq (M,T) int64, seq_mask (M,T) -- per row.  cap_classes (M,T) int64 and class_mask (M,T) likewise.
 *
 * The encoder, init_hidden and v2a(V) run once on the B videos; only the initial state is repeated to the M rows.  Every step's
 * attention, forward and backward, reads a video's V and v2a(V) at row / Q.  The loss is LanguageModelCriterion + weight_class *
 * ClassiferCriterion over the M rows.  Train-mode BatchNorm takes its batch statistics from the B videos (they equal those of the
 * row-repeated batch) and makes ONE momentum update of the running statistics, with the unbiased factor over B K samples.  Dropout:
 * the encoder's sites draw by element index in the B-video tensors, the decoder's and the heads' by row in the M-row tensors.
 *
 * The backward sums what a video's Q rows send to its V, v2a(V) and initial state with ONE writer per element and the Q T terms in
 * a fixed order (no float atomics on them), then runs the encoder's backward on the B videos.
 */
#ifndef XGATE_TRAIN_VIDEO_H
#define XGATE_TRAIN_VIDEO_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGTV_VERSION 1

int xgtv_version(void);
/* bytes of the workspace at dims d (d->B = VIDEOS) with Q rows per video: the per-video encoder part and the (B Q)-row decoder part
 * with every per-step tensor the backward reads, in one block; 0 for invalid dims, Q < 1, or B * Q beyond 2^20 rows.  Of the row
 * part only the attention weights and their gradients are of size (rows, K): no (rows, K, R) or (rows, K, A) tensor. */
size_t xgtv_workspace_bytes(const XgDims *d, int32_t Q);

/*
 * losses[0..2] (device) = total, language-model and classifier loss, as xg_xe_loss_fwd leaves them.  cap_classes == NULL: no
 * classifier term (class_mask and weight_class are then not read).  run->save is not read: the workspace always holds what
 * xgtv_xe_loss_bwd needs.
 * XG_EINVAL, before anything is enqueued: invalid dims, Q < 1, B * Q beyond 2^20 or a null workspace; then, behind the size test
 * below: a workspace that is not 256-byte aligned, a null pointer (p, x and its six fields, run, losses; in eval mode bn and its
 * four statistics), a run->gemm_mode other than 0.
 * XG_EWORKSPACE: ws_bytes below xgtv_workspace_bytes(d, Q).
 */
int xgtv_xe_loss_fwd(void *stream, const XgDims *d, int32_t Q, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                     const int64_t *cap_classes, const float *class_mask, float weight_class, const XgRun *run, void *ws,
                     size_t ws_bytes, float *losses);
/*
 * g += dloss_dev[0] * d(losses[0]) / d(parameter) for every parameter, from the workspace xgtv_xe_loss_fwd left, with the same
 * d, Q, x, cap_classes, class_mask, weight_class and run (run->grad_event / grad_event_head as in xg_xe_loss_bwd).  The gates are
 * those of the forward (g and dloss_dev among the pointers).
 */
int xgtv_xe_loss_bwd(void *stream, const XgDims *d, int32_t Q, const XgParams *p, const XgParams *g, const XgBatch *x,
                     const int64_t *cap_classes, const float *class_mask, float weight_class, const float *dloss_dev,
                     const XgRun *run, void *ws, size_t ws_bytes);
/*
 * For tests and tools, behind xgtv_xe_loss_bwd on the same workspace: the per-video sums over a video's Q rows and the T steps,
 * formed again from the saved per-step tensors into the caller's buffers --
 *   dvproj (B,K,A) = sum_t sum_q de[t, b Q + q, k] * w_a * (1 - tanh^2(P[t, b Q + q, a] + v2a(V)[b, k, a]))
 *   dV (B,K,R)     = sum_t sum_q alpha[t, b Q + q, k] * dAF[t, b Q + q, r]      (the attention's share: without dvproj W_v2a)
 * Same gates as above (p: only a2w.weight is read).
 */
int xgtv_video_grads(void *stream, const XgDims *d, int32_t Q, const XgParams *p, void *ws, size_t ws_bytes, float *dvproj,
                     float *dV);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_TRAIN_VIDEO_H */
