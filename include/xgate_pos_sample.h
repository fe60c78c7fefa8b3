/*
 * xgate_pos_sample.h -- C ABI of SAMPLED POS templates in libxgate_hip.so (gfx950): the rollout of pos_src/SAModel.py:136-184
 * with the torch.max choice replaced by a draw from the head's distribution, S rollouts for each of B videos.  What it writes
 * to `templates` is directly a valid input of xgpc_sample_forced (xgate_pos_control.h), and the state it ends in is the
 * captioner's `pos_feats`: the generator proposes the syntactic plans itself and a video is captioned under each.
 *
 * Eval mode, fp32.  The conventions are those of xgate_pos_control.h: device pointers, caller-owned memory, d->B counts VIDEOS,
 * d->T = seq_length + 1 = L + 1 decoder steps, one row is one (video b, rollout s) pair with row index b * S + s, every entry
 * point only ENQUEUES work on `stream`, arguments are checked before anything is enqueued, and a call does not depend on what
 * the workspace held before.  No random number generator lives in the library: the caller supplies one uniform in [0, 1] per
 * draw, as with the captioner's xg_rollout (xgate.h).
 */
#ifndef XGATE_POS_SAMPLE_H
#define XGATE_POS_SAMPLE_H

#include "xgate_pos_control.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPS_VERSION 1

int xgps_version(void);
/* bytes of the workspace of xgps_sample_templates at dims d with S rollouts per video; 0 for invalid dims, S < 1 or B * S
 * rows beyond 32-bit offsets */
size_t xgps_workspace_bytes(const XgpDims *d, int32_t S);

/*
 * Sampled rollout.  Step 0 feeds BOS (0) with mask 1.  At the end of step t - 1 (1 <= t <= L) the head holds the C logits x,
 * and the tag of step t is drawn by inverse CDF (the captioner's rule, caption_src/SAModel.py:189-195):
 *     w_c = exp((x_c - max x) / temperature),  target = uniforms[b,s,t-1] * sum(w),
 *     tag_t = the first c, in category order, whose running sum of w exceeds target; C - 1 when none does.
 * unfinished_t = unfinished_{t-1} * (tag_t > 0) is the mask of step t: finished rows hold h and c exactly.
 *   uniforms (B,S,L)      one uniform per draw, in [0, 1]
 *   templates (B,S,L)     int64 out: tag_t * unfinished_t at [.., t-1], so a row is zero from its first 0 onwards
 *   tag_logp (B,S,L)      the UNTEMPERED log_softmax(x)[tag_t] at [.., t-1] while the row was unfinished before the draw (up to
 *                         and including its first 0), 0.0 after it; the row sum is the template's score, as in the forced call
 *   states, masks, pos_feats, n_out: exactly as in xgpc_sample_forced (states may be NULL: not stored)
 * All L + 1 steps run on the device.  XG_EINVAL: a temperature that is not finite or <= 0, S < 1, a null pointer other than
 * `states`, invalid dims; XG_EWORKSPACE: ws_bytes below xgps_workspace_bytes(d, S).
 */
int xgps_sample_templates(void *stream, const XgpDims *d, int32_t S, float temperature, const XgpParams *p,
                          const XgBnState *bn, const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                          const float *uniforms, int64_t *templates, float *tag_logp, float *states, float *masks,
                          float *pos_feats, int32_t *n_out, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_SAMPLE_H */
