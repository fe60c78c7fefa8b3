/*
 * xgate_pos_train.h -- C ABI for training the POS sequence generator in libxgate_hip.so (gfx950): the teacher-forced
 * iteration of the reference's pos_src/starttrain_trainpos.py:138-152 (train-mode forward, backward), fp32, one GPU.
 *
 * The conventions are those of xgate_pos.h (dimension names, XgpDims, XgpParams, XG_E* codes):
 *   - all tensor pointers are DEVICE pointers, fp32 unless noted, row-major and contiguous in the documented shape;
 *   - the caller owns all memory: the saved activations of a forward live in one caller-provided workspace sized by
 *     xgpt_workspace_bytes() (no zero-fill needed);
 *   - every entry point only ENQUEUES work on `stream` and returns; arguments are checked before anything is enqueued.
 *
 * A backward reads what the LAST forward_train on the same workspace saved: the caller pairs them (a second forward
 * on the workspace overwrites the first one's activations).
 */
#ifndef XGATE_POS_TRAIN_H
#define XGATE_POS_TRAIN_H

#include "xgate_pos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPT_VERSION 1

/* Train shapes are limited beyond xgate_pos.h's: T * K * sizeof(float) must not exceed XGPT_MAX_TK_BYTES (the attention
 * backward holds a video's T x K score gradients in LDS), e.g. K <= 517 frames at seq_length 28 (T = 29).
 * xgpt_workspace_bytes returns 0 and xgpt_forward_train XG_EINVAL for d->T * d->K beyond it, xgpt_backward for Tp * d->K. */
#define XGPT_MAX_TK_BYTES 60000

/* train != 0: BatchNorm with batch statistics (running statistics updated in place: running = (1 - bn_momentum) running
 * + bn_momentum batch, unbiased variance) and hash dropout with probability drop_p (oracle/paramgen.py:keep_mask, sites
 * 0 rgb embedding, 1 opfl embedding, 4 fusion, 6 decoder cell at step t).  train == 0: eval-mode BatchNorm over the
 * running statistics and no dropout (activations are still saved). */
typedef struct XgptRun {
    int32_t train;
    float drop_p;
    uint32_t seed;
    float bn_momentum;
} XgptRun;

int xgpt_version(void);
/* bytes of the training workspace at dims d (d->T = cap_classes.size(1)); 0 for invalid dims */
size_t xgpt_workspace_bytes(const XgpDims *d);

/* Train-mode teacher-forced forward (pos_src/SAModel.py:62-90): the inputs of xgp_forward_tf; logp (B,T,C) receives
 * the log-probabilities of all T steps and t_out (device int32[1]) T' (only logp[:, :T'] is the reference's output).
 * bn: running statistics, updated in place when run->train.  The activations are saved into ws. */
int xgpt_forward_train(void *stream, const XgpDims *d, const XgpParams *p, const XgBnState *bn, const XgptRun *run,
                       const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                       const int64_t *cap_classes, const float *new_mask,
                       float *logp, int32_t *t_out, void *ws, size_t ws_bytes);

/* Backward of the last forward_train on ws over its first Tp (1 <= Tp <= d->T) steps: dlogp (B,Tp,C) is the gradient
 * of the loss wrt logp[:, :Tp].  run, the features and the mask are those of the forward.  The gradients are ADDED to
 * the buffers of g (one per parameter, XgpParams order; every pointer must be non-null). */
int xgpt_backward(void *stream, const XgpDims *d, const XgpParams *p, const XgpParams *g, const XgptRun *run,
                  const float *feats_rgb, const float *feats_opfl, const float *feat_mask, int32_t Tp,
                  const float *dlogp, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_TRAIN_H */
