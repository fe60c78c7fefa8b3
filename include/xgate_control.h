/*
 * xgate_control.h -- C ABI of the captioner's rollout over MANY `pos_feats` ROWS PER VIDEO in libxgate_hip.so (gfx950): what
 * controllable_xgating_amd/control.py runs when a video is captioned under S POS templates, on one shared encoder pass.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h and xgate_beam.h: device pointers, caller-owned memory, every entry point
 * only ENQUEUES work on `stream`, arguments are checked before anything is enqueued, and a call does not depend on what the
 * workspace held before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1, one row is one (video b, template s) pair with row
 * index b * S + s.  The encoder, init_hidden and v2a(V) run once on the B videos and are NOT row-repeated: only the initial state
 * (4 B S R floats) is.  The attention of a step reads a video's v2a(V) and V once for every group of XGCC_TEMPLATE_GROUP of its
 * rows; no step needs the host.
 */
#ifndef XGATE_CONTROL_H
#define XGATE_CONTROL_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGCC_VERSION 1

/* rows of one video that one workgroup of the step's attention serves; a video's last group may be partial */
#define XGCC_TEMPLATE_GROUP 4

int xgcc_version(void);
/* bytes of the workspace of xgcc_rollout at dims d (d->B = VIDEOS) with S rows per video: the per-video encoder part and the
 * (B S)-row step part in one block; 0 for invalid dims (d->T < 2 among them), S < 1, or B * S beyond 2^20 rows */
size_t xgcc_workspace_bytes(const XgDims *d, int32_t S);

/*
 * xg_rollout in eval mode on the batch in which video b is repeated S times, taken row by row: the same token choice (greedy
 * argmax, or the draw from softmax(logits / temperature) by uniforms[t][row] with the log-probability gathered UNTEMPERED), the
 * same `unfinished` bookkeeping and n_steps, and the reference's dead last step is not run.
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (B*S,R), row
 *                         b * S + s; seq / seq_mask are not read
 *   mode                  XG_ROLLOUT_GREEDY or XG_ROLLOUT_SAMPLE
 *   uniforms (T, B*S)     SAMPLE mode only
 *   seq (B*S,L)           int64 out, written in full (zero after a row's finish)
 *   seq_logp (B*S,L)      written in full
 *   n_steps               int32 out: the reference's early-exit length
 * XG_EINVAL, before anything is enqueued: invalid dims, S < 1, B * S beyond 2^20, a null pointer (bn and its four statistics
 * included: eval mode reads them), run->train, run->save, a run->gemm_mode other than 0, a mode other than the two above (replay
 * among them), SAMPLE mode without uniforms or with temperature <= 0, a workspace that is not 256-byte aligned.
 * XG_EWORKSPACE: ws_bytes below xgcc_workspace_bytes(d, S).
 */
int xgcc_rollout(void *stream, const XgDims *d, int32_t S, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                 const XgRun *run, int mode, const float *uniforms, float temperature, int64_t *seq, float *seq_logp,
                 int32_t *n_steps, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_CONTROL_H */
