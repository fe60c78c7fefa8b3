/*
 * xgate_pos_control.h -- C ABI of controlled generation with the POS sequence generator in libxgate_hip.so (gfx950):
 * the rollout of pos_src/SAModel.py:136-184 with the greedy choice replaced by the caller's tag sequence (a POS
 * template), S templates for each of B videos.  The state it ends in is the captioner's `pos_feats`
 * (caption_src/data_io.py:215-217), so a video is captioned under a chosen template.
 *
 * Eval mode, fp32.  The conventions are those of xgate_pos.h (dimension names, XgpDims, XgpParams, XgBnState, XG_E*
 * codes): device pointers, caller-owned memory, every entry point only ENQUEUES work on `stream`, arguments are checked
 * before anything is enqueued, and a call does not depend on what the workspace held before.
 *
 * d->B counts VIDEOS and d->T = seq_length + 1 = L + 1 decoder steps.  One row is one (video b, template s) pair, row
 * index b * S + s.  The encoder, init_hidden, v2a(V) and the token table run once over the B videos; the decoder steps run
 * over the B * S rows, and the attention of a step reads a video's v2a(V) and V once for a group of
 * XGPC_TEMPLATE_GROUP of its templates.
 */
#ifndef XGATE_POS_CONTROL_H
#define XGATE_POS_CONTROL_H

#include "xgate_pos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPC_VERSION 1

/* templates of one video that one workgroup of the step's attention serves (a last group may be partial) */
#define XGPC_TEMPLATE_GROUP 4

int xgpc_version(void);
/* bytes of the workspace of xgpc_sample_forced at dims d with S templates per video; 0 for invalid dims, S < 1 or
 * B * S rows beyond 32-bit offsets */
size_t xgpc_workspace_bytes(const XgpDims *d, int32_t S);

/*
 * Forced rollout.  templates (B,S,L) int64: entry t - 1 is the tag fed at step t (1 <= t <= L); step 0 feeds BOS (0)
 * with mask 1.  unfinished_t = unfinished_{t-1} * (tag_t > 0) is the mask of step t, so the step that feeds a row's
 * first 0 and every later one hold h and c exactly: tags after the first 0 are ignored.  Tags outside [0, C) are
 * clamped into it, silently: a tag >= C is fed and scored as C - 1 (a live tag), a negative tag as 0 (it ENDS the
 * template), so tag_logp and the template's score of such a row belong to the clamped tags, not to the ones passed.
 * A caller that cannot vouch for its tags checks them first (the Python layer does for lists and host tensors).
 *   tag_logp (B,S,L)      log_softmax(logit(h_{t-1}))[tag_t] at [.., t-1] for every t up to and including the row's
 *                         first 0, 0.0 after it; the row sum is the template's score
 *   states (B,S,L+1,R)    h after each step; NULL: not stored
 *   masks (B,S,L+1)       the mask of each step
 *   pos_feats (B*S,R)     h after the last step (= states[:, :, n] for the n below: finished rows hold)
 *   n_out (device int32[1]) min(L, the largest number of leading non-zero tags of a row): the reference's n; 0 when
 *                         every template is empty
 * All L + 1 steps run on the device.
 */
int xgpc_sample_forced(void *stream, const XgpDims *d, int32_t S, const XgpParams *p, const XgBnState *bn,
                       const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                       const int64_t *templates, float *tag_logp, float *states, float *masks,
                       float *pos_feats, int32_t *n_out, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_CONTROL_H */
