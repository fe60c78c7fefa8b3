/*
 * xgate_score.h -- C ABI of SCORING GIVEN CAPTIONS in libxgate_hip.so (gfx950): the log-probability the captioner gives each token
 * of a caption it is handed, Q caption rows per video on one shared encoder pass.  What SAModel.score_captions_per_video runs:
 * reranking a video's candidate captions, template recovery (a caption under every POS template), per-reference likelihood.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h: device pointers, caller-owned memory, the entry point only ENQUEUES work
 * on `stream`, arguments are checked before anything is enqueued, and the call does not depend on what the workspace held before.
 * d->B counts VIDEOS, d->T = seq_length + 1 = L + 1.  One row is one (video b, pos_feats row, caption) triple with row index
 * b * Q + q.  The encoder, init_hidden and v2a(V) run once on the B videos and are NOT row-repeated: only the initial state is.  A
 * step's attention reads a video's v2a(V) and V once per group of its rows.  The time loop is L decoder steps and nothing else: the
 * tokens are known up front, so the vocabulary scoring of finished steps runs in chunks of whole steps beside the loop (on the side
 * stream of run->aux when there is one).  The (rows, V) logits are never written: the scoring kernel leaves a row's log-sum-exp
 * statistics and its target's logit only.
 *
 * Result of a row = what the teacher-forced replay of `tokens` gives (SAModel.sample with forced tokens, row by row, on the batch
 * with each video repeated Q times):
 *   tok_logp[j]   the untempered log-probability of tokens[j] at step j, kept for the COUNTED columns only: column 0 and every
 *                 column whose preceding tokens are all non-zero (zero = EOS; the first EOS is counted); 0 in every other column
 *   count         the number of counted columns, 1 .. L
 *   score         the sum of tok_logp over the counted columns
 * Token values are clamped into [0, V) by the kernels; nothing is read back on the host.
 */
#ifndef XGATE_SCORE_H
#define XGATE_SCORE_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGSC_VERSION 1

int xgsc_version(void);
/* bytes of the workspace of xgsc_score_captions at dims d (d->B = VIDEOS) with Q rows per video: the per-video encoder part and the
 * (B Q)-row step part in one block; 0 for invalid dims (d->T < 2 among them), Q < 1, or B * Q beyond 2^20 rows.  It holds no
 * (rows, V) tensor: a further row costs less than one row of logits. */
size_t xgsc_workspace_bytes(const XgDims *d, int32_t Q);

/*
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (B*Q,R), row
 *                         b * Q + q; seq / seq_mask are not read
 *   tokens (B*Q, L)       int64, zero = EOS, zero-padded
 *   tok_logp (B*Q, L)     out, written in full
 *   score (B*Q)           out
 *   count (B*Q)           int32 out
 * XG_EINVAL, before anything is enqueued: invalid dims, Q < 1, B * Q beyond 2^20 or a null workspace; then, behind the size test
 * below: a workspace that is not 256-byte aligned, a null pointer (bn and its four statistics included: eval mode reads them),
 * run->train, run->save, a run->gemm_mode other than 0.
 * XG_EWORKSPACE: ws_bytes below xgsc_workspace_bytes(d, Q).
 */
int xgsc_score_captions(void *stream, const XgDims *d, int32_t Q, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                        const XgRun *run, const int64_t *tokens, float *tok_logp, float *score, int32_t *count, void *ws,
                        size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_SCORE_H */
