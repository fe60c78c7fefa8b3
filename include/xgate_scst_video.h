/*
 * xgate_scst_video.h -- C ABI of SELF-CRITICAL TRAINING ON S ROLLOUTS PER VIDEO in libxgate_hip.so (gfx950): the sampled rollout of
 * xg_rollout (xgate.h) and its backward xg_rollout_bwd with the B videos handed over ONCE and S rollout rows each, and the
 * policy-gradient criterion over the B x S rows with the advantage formed on the device.  What SAModel.rollout_per_video and
 * PerVideoRewardCriterion run.
 *
 * fp32 data path (XgRun.gemm_mode 0), train and eval mode.  The conventions are those of xgate_train_video.h: device pointers,
 * caller-owned memory, the entry points only ENQUEUE work on `stream`, arguments are checked before anything is enqueued, and no call
 * depends on what the workspace held before the forward.  d->B counts VIDEOS, d->T = seq_length + 1, L = d->T - 1.  Row b * S + s is
 * rollout s of video b; M = B S rows.
 *
 *   x   feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (M,R) per row.
 *
 * The encoder, init_hidden and v2a(V) run once on the B videos; only the initial state is repeated to the M rows.  Every step's
 * attention, forward and backward, reads a video's V and v2a(V) at row / S.  Train-mode BatchNorm takes its batch statistics from the
 * B videos and makes ONE momentum update of the running statistics, with the unbiased factor over B K samples.  Dropout: the
 * encoder's sites draw by element index in the B-video tensors, the decoder's by row in the M-row tensors.
 */
#ifndef XGATE_SCST_VIDEO_H
#define XGATE_SCST_VIDEO_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGSV_VERSION 1

/* how xgsv_reward_fwd forms the advantage of row (b, s) from score (B,S) */
#define XGSV_BASE_NONE 0        /* adv = score                                                                                  */
#define XGSV_BASE_MEAN_OTHERS 1 /* adv = score[b,s] - (sum of the video's other S - 1 scores, added in index order) / (S - 1)   */
#define XGSV_BASE_GIVEN 2       /* adv = score[b,s] - base[b]                                                                    */

int xgsv_version(void);
/* bytes of the workspace at dims d (d->B = VIDEOS) with S rows per video: the per-video encoder part and the (B S)-row part with
 * every per-step tensor the backward reads, in time-major blocks, and the rollout's own buffers; 0 for invalid dims, S < 1, or
 * B * S beyond 2^20 rows.  No classifier tensors.  Of the row part only the attention weights and their gradients are of size
 * (rows, K): no (rows, K, R) or (rows, K, A) tensor. */
size_t xgsv_workspace_bytes(const XgDims *d, int32_t S);

/*
 * The SAMPLE-mode xg_rollout, row by row, on the batch in which video b is repeated S times: uniforms (T, M), one per step and
 * row; a token is drawn from softmax(logits / temperature), seq_logp gathers the UNTEMPERED log-probability.  seq (M, L) int64,
 * seq_logp (M, L) and n_steps[0] (the early-exit width) as xg_rollout leaves them: every element is written.  run->save is not
 * read: the workspace always holds what xgsv_rollout_bwd needs.
 * XG_EINVAL, before anything is enqueued: invalid dims, S < 1, B * S beyond 2^20 or a null workspace; then, behind the size test
 * below: a workspace that is not 256-byte aligned, a null pointer (p, x and its four fields, run, uniforms, seq, seq_logp, n_steps;
 * in eval mode bn and its four statistics), a temperature that is not positive, a run->gemm_mode other than 0.
 * XG_EWORKSPACE: ws_bytes below xgsv_workspace_bytes(d, S).
 */
int xgsv_rollout(void *stream, const XgDims *d, int32_t S, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                 const XgRun *run, const float *uniforms, float temperature, int64_t *seq, float *seq_logp, int32_t *n_steps,
                 void *ws, size_t ws_bytes);
/*
 * g += sum over rows and steps of dseq_logp[row, t] * d(seq_logp[row, t]) / d(parameter), from the workspace xgsv_rollout left, with
 * the same d, S, x and run (run->grad_event / grad_event_head as in xg_xe_loss_bwd).  dseq_logp (M, L).  The gates are those of the
 * rollout (g and dseq_logp among the pointers).  What a video's S rows send to its V, v2a(V) and initial state is summed with ONE
 * writer per element in a fixed order.
 */
int xgsv_rollout_bwd(void *stream, const XgDims *d, int32_t S, const XgParams *p, const XgParams *g, const XgBatch *x,
                     const XgRun *run, const float *dseq_logp, void *ws, size_t ws_bytes);

/*
 * RewardCriterion over the B x S rows with one score per row.  seq_logp, seq (M, L) contiguous; score (B, S); base (B) for
 * XGSV_BASE_GIVEN, else not read; n_dev: the rollout's n_steps (device int32, may be null: L).  Writes advantage (B, S) and
 * out[0..1] = { sum -seq_logp * adv * mask, sum mask } with mask[row, 0] = 1, mask[row, t] = seq[row, t - 1] > 0, columns t >= n
 * masked out.  partial (B, 2) is scratch: one workgroup per video writes its pair, one pass adds the B pairs in index order -- no
 * float atomics, no zeroed output, two identical calls give identical bits.
 * XG_EINVAL: a null pointer, B, S or L < 1, B * S beyond 2^20, L beyond 2^10, an unknown baseline, XGSV_BASE_MEAN_OTHERS with S < 2,
 * XGSV_BASE_GIVEN without base.
 */
int xgsv_reward_fwd(void *stream, const float *seq_logp, const int64_t *seq, const float *score, const float *base,
                    int32_t baseline, const int32_t *n_dev, int32_t B, int32_t S, int32_t L, float *advantage, float *partial,
                    float *out);
/* dseq_logp (M, L) = -scale * advantage[row] * mask / sums[1]; sums: xgsv_reward_fwd's out; scale_dev (device float, null: 1). */
int xgsv_reward_bwd(void *stream, const int64_t *seq, const float *advantage, const int32_t *n_dev, int32_t B, int32_t S,
                    int32_t L, const float *sums, const float *scale_dev, float *dseq_logp);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_SCST_VIDEO_H */
