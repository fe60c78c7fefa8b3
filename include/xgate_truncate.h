/*
 * xgate_truncate.h -- C ABI of the captioner's TRUNCATED sampling rollout in libxgate_hip.so (gfx950): top-k and nucleus (top-p)
 * draws over S `pos_feats` rows per video, on one shared encoder pass.  What SAModel.sample_truncated_per_video runs.
 *
 * Eval mode, fp32.  The conventions, the row layout (row b * S + s) and the workspace are those of xgate_control.h: this is
 * that header's rollout in SAMPLE mode with every choice t >= 1 made by the truncated draw of docs/CAPTION_TRUNCATED.md instead of the
 * plain multinomial one.  No step needs the host.
 */
#ifndef XGATE_TRUNCATE_H
#define XGATE_TRUNCATE_H

#include "xgate_control.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGTR_VERSION 1

int xgtr_version(void);
/* bytes of the workspace of xgtr_rollout: the size xgate_control.h gives for (d, S) -- the truncated draw needs nothing of its own */
size_t xgtr_workspace_bytes(const XgDims *d, int32_t S);

/*
 * A draw of row r at step t from the raw logits x (V) of the previous step:
 *   w_v = exp((x_v - max x) / temperature)
 *   top_k (0 or >= V: off)   keeps {v : x_v >= the top_k-th largest value of x}, ties at that value included
 *   top_p (1: off)           inside that set, of mass Z_k: keeps {v : x_v >= y} for the largest y occurring in x whose set has
 *                            mass >= top_p * Z_k -- whole classes of equal values, so the kept set K never depends on column order
 *   the token                the first column, in column order, whose running sum of w_v [v in K] exceeds uniforms[t][r] * Z_K
 * The `unfinished` bookkeeping, n_steps and the dead last step are those of xgate_control.h.
 *   x, run                as in xgate_control.h
 *   uniforms (T, B*S)     required
 *   seq (B*S,L)           int64 out, written in full (zero after a row's finish)
 *   seq_logp (B*S,L)      x_tok - lse(x): the UNTEMPERED, UNTRUNCATED log-probability, written in full
 *   seq_logq (B*S,L)      log(w_tok / Z_K), the log-probability under the distribution sampled from; 0 after a row's end token;
 *                         may be null
 *   kept (B*S,L)          int32 |K|; 0 after a row's end token; may be null
 *   n_steps               int32 out: the reference's early-exit length
 * XG_EINVAL, before anything is enqueued: whatever the rollout of xgate_control.h refuses, top_k < 0, top_p outside (0, 1], null uniforms,
 * temperature <= 0.  XG_EWORKSPACE: ws_bytes below xgtr_workspace_bytes(d, S).
 */
int xgtr_rollout(void *stream, const XgDims *d, int32_t S, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                 const XgRun *run, int32_t top_k, float top_p, const float *uniforms, float temperature, int64_t *seq,
                 float *seq_logp, float *seq_logq, int32_t *kept, int32_t *n_steps, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_TRUNCATE_H */
