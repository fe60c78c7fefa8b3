/*
 * xgate_pair.h -- C ABI of the SCST rollout pair under TRAIN-MODE DROPOUT in libxgate_hip.so (gfx950): the sampled rollout and the
 * greedy baseline of one self-critical iteration as ONE decoder loop over 2m rows, each half under its OWN dropout realisation --
 * what controllable_xgating_amd.SAModel.sample_pair(..., {"one_pass": True}) runs when drop_prob_lm > 0 (docs/SCST_DROPOUT.md).
 *
 * The conventions are those of xgate.h: device pointers, caller-owned memory, the entry point only ENQUEUES work on `stream`,
 * arguments are checked before anything is enqueued, and the call does not depend on what either workspace held before.
 *
 * Every dropout mask of the library is a stateless hash of (seed, site, step, element).  Rows [0, m) -- the sampled half -- take
 * run->seed with the element indices of an m-row call; rows [m, 2m) -- the greedy half -- take seed_greedy with the element
 * indices of rows [0, m) of a call of THEIR own.  So the two halves compute what xg_rollout computes for the m videos in SAMPLE
 * mode under run->seed and in GREEDY mode under seed_greedy, and xg_rollout_bwd on ws1 under run->seed regenerates the masks of
 * the sampled half.  The encoder, init_hidden and v2a(V) run once per seed on the m videos (their dropout sites differ between the
 * halves too), each pass with its own BatchNorm running-statistics update: two updates with the statistics of the m-row batch.
 */
#ifndef XGATE_PAIR_H
#define XGATE_PAIR_H

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPR_VERSION 1

int xgpr_version(void);

/*
 * xg_rollout_pair_videos (xgate.h) with a second dropout seed: every argument means what it means there.
 *   d2, d1                d2->B = 2 m rows, d1->B = m videos, all other dims equal
 *   x1                    the m videos ONCE: feats_rgb, feats_opfl, feat_mask, pos_feats (m,R)
 *   run                   run->seed: the sampled half's seed (and the one xg_rollout_bwd on ws1 takes)
 *   seed_greedy           the greedy half's seed; seed_greedy == run->seed is valid: both halves then draw the same masks
 *   uniforms (T, m)       the sampled half's draws
 *   ws2 / ws1             workspaces of xg_workspace_bytes[_mode] at d2 / d1, distinct.  The encoder pass under run->seed runs in
 *                         ws1 (where the backward reads it), the one under seed_greedy in the row prefix of ws2; no third workspace
 *   compact               non-zero: the sampled half's activations end up in ws1 for xg_rollout_bwd(d1, ..., ws1)
 *   seq, seq_logp (2m,L)  rows [0, m) sampled, rows [m, 2m) greedy, written in full
 *   n_steps               int32[2]: the two rollouts' early-exit lengths
 * With run->train == 0 or run->drop_p == 0 no site drops and the call computes what xg_rollout_pair_videos computes, except that
 * the encoder runs twice.
 * XG_EINVAL, before anything is enqueued: whatever xg_rollout_pair_videos refuses -- invalid or unequal dims, d2->B != 2 d1->B,
 * ws1 == ws2, a null pointer (uniforms and the three outputs among them), temperature <= 0, a workspace that is not 256-byte
 * aligned.  XG_EWORKSPACE: ws2_bytes / ws1_bytes below the size at d2 / d1.
 */
int xgpr_rollout_pair_videos(void *stream, const XgDims *d2, const XgParams *p, const XgBnState *bn, const XgBatch *x1,
                             const XgRun *run, uint32_t seed_greedy, const float *uniforms, float temperature, void *ws2,
                             size_t ws2_bytes, const XgDims *d1, void *ws1, size_t ws1_bytes, int compact, int64_t *seq,
                             float *seq_logp, int32_t *n_steps);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_PAIR_H */
