/*
 * xgate_pos_beam_diverse.h -- C ABI of DIVERSE POS BEAM SEARCH in libxgate_hip.so (gfx950): diverse beam search (Vijayakumar et
 * al. 2016, Hamming diversity) over the POS generator.  The W best templates of the plain search (xgate_pos_beam.h) differ in one
 * tag; here a video's N = Gd * Wg slots are split into Gd groups of Wg, each group is a beam search of width Wg by the plain rule,
 * and a group is steered away from the tags the groups before it took at the same step.  What it writes to `templates`, read as
 * (B, N, L), is directly a valid input of xgpc_sample_forced (xgate_pos_control.h) at S = N.
 *
 * Eval mode, fp32.  The conventions are those of xgate_pos_beam.h: device pointers, caller-owned memory, d->B counts VIDEOS,
 * d->T = seq_length + 1 = L + 1, one row is one (video b, slot) pair with row index b * N + slot, group j owns slots
 * j * Wg .. (j + 1) * Wg - 1, every entry point only ENQUEUES work on `stream`, arguments are checked before anything is enqueued,
 * and a call does not depend on what the workspace held before.  No step needs the host: a video's whole merge runs in one
 * workgroup, its groups in series.
 */
#ifndef XGATE_POS_BEAM_DIVERSE_H
#define XGATE_POS_BEAM_DIVERSE_H

#include "xgate_pos_beam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGPD_VERSION 1

/* the most slots per video: Gd * Wg <= XGPD_MAX_BEAM (= XGPB_MAX_BEAM) */
#define XGPD_MAX_BEAM 8

/* LDS bytes of a video's merge workgroup: XGPB_LDS_BYTES at W = N, with 1536 bytes of fixed tables (the plain merge's, the
 * unpenalised log-probabilities of the candidates, the video's parents and the penalty list) */
#define XGPD_LDS_BYTES(N, R, C) (4 * (size_t)(N) * (2 * (size_t)(R) + (size_t)(C)) + 1536)
#define XGPD_MAX_LDS_BYTES 65536

int xgpd_version(void);
/* bytes of the workspace of xgpd_beam_templates at dims d with Gd groups of Wg slots; 0 for whatever that call refuses with
 * XG_EINVAL on account of d, Gd and Wg */
size_t xgpd_workspace_bytes(const XgpDims *d, int32_t Gd, int32_t Wg);

/*
 * Diverse beam search.  Every group is the search of xgpb_beam_templates at W = Wg (its steps 1-5), with its own running sums, its
 * own done list of Wg entries and its own ranking.  Within step t the groups of a video are merged in the order j = 0 .. Gd-1,
 * with one change to step 3:
 *   n_j(c) = the number of new slots of groups 0 .. j-1 at step t that are LIVE (their new sum p > -500) and hold tag c.  Tag 0
 *            counts like any other; dead slots never count.
 *   a[q][c] = lp[q][c] - lambda * n_j(c) for every row q of group j: in fp32 one multiply ((float)n * lambda) and one subtraction,
 *            each rounded on its own (no FMA).  lp carries the -1000 of suppress_tag.
 *   Step 3 runs over a: row q contributes its Wg best a, lower tag first on exact ties; candidate c_rank * rows + q carries
 *   p = sum[q] + a (one fp32 add); the first Wg of the stable descending sort are the group's new slots.  At t = 0 a group has one
 *   row, so at lambda > 0 the groups already open with different tags.
 * sum = p carries the penalties; the r stored for the tag is the UNPENALISED lp.  A beam's score is its penalised sum at the
 * moment it finished (what its group ranked by); tag_logp summed gives the pure sum.  Steps 4-5 per group are unchanged.
 * Gd = 1 is xgpb_beam_templates at W = Wg bit for bit, whatever lambda; at lambda = 0 every group equals that search.
 *   templates (B,Gd,Wg,L)  int64 out: a group's done beams, best first, zero after a beam's finish
 *   tag_logp (B,Gd,Wg,L)   their unpenalised r, zero after the finish
 *   score (B,Gd,Wg)        their penalised p
 *   masks (B,Gd,Wg,L+1)    column 0 is 1, column t is 1 while the first t tokens are all non-zero
 *   n_out (device int32[1]) from masks as in xgpc_sample_forced; 0 is legal
 *   trace (B,L,N,2)        int32 (token, parent) of every slot and step; the parent is a slot index of the VIDEO, 0 .. N-1, and
 *                          lies in the slot's own group (at t = 0 it is j * Wg); NULL: not stored
 * XG_EINVAL, before anything is enqueued: Gd < 1, Wg < 1, Gd * Wg > C, Gd * Wg > XGPD_MAX_BEAM, suppress_tag >= C,
 * XGPD_LDS_BYTES(Gd * Wg, R, C) > XGPD_MAX_LDS_BYTES, lambda negative, infinite or NaN, a null pointer other than `trace`, invalid
 * dims (those of xgpc_sample_forced at S = Gd * Wg).  XG_EWORKSPACE: ws_bytes below xgpd_workspace_bytes(d, Gd, Wg).
 */
int xgpd_beam_templates(void *stream, const XgpDims *d, int32_t Gd, int32_t Wg, float lambda, int32_t suppress_tag,
                        const XgpParams *p, const XgBnState *bn, const float *feats_rgb, const float *feats_opfl,
                        const float *feat_mask, int64_t *templates, float *tag_logp, float *score, float *masks, int32_t *n_out,
                        int32_t *trace, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_BEAM_DIVERSE_H */
