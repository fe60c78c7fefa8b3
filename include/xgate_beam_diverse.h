/*
 * xgate_beam_diverse.h -- C ABI of the CAPTIONER'S DIVERSE BEAM SEARCH in libxgate_hip.so (gfx950): diverse beam search (Vijayakumar
 * et al. 2016, Hamming diversity) under S POS templates per video, on one shared encoder pass.  The W best captions of the plain
 * search differ in one word near the end; here the N = Gd * Wg slots of a (video, template) pair are split into Gd groups of Wg,
 * each group is a beam search of width Wg by the plain rule, and a group is steered away from the words the groups before it
 * took at the same step.
 *
 * Eval mode, fp32.  The conventions are those of xgate_beam_control.h: device pointers, caller-owned memory, every entry point only
 * ENQUEUES work on `stream`, arguments are checked before anything is enqueued, and a call does not depend on what the workspace
 * held before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1.  A PAIR is one (video b, template s), pair = b * S + s; group j
 * of a pair owns its slots j * Wg .. (j + 1) * Wg - 1; one row is one (pair, slot) with row index pair * N + slot.  The encoder,
 * init_hidden and v2a(V) run once on the B videos; no step needs the host.
 */
#ifndef XGATE_BEAM_DIVERSE_H
#define XGATE_BEAM_DIVERSE_H

#include "xgate_beam_control.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGDB_VERSION 1

/* the most slots per pair, Gd * Wg <= XGDB_MAX_BEAM: the widest beam of xgate_beam.h */
#define XGDB_MAX_BEAM 8

int xgdb_version(void);
/* bytes of the workspace of xgdb_beam_search at dims d (d->B = VIDEOS) with S templates per video and Gd groups of Wg slots per
 * pair; 0 for whatever that call refuses with XG_EINVAL on account of d, S, Gd and Wg */
size_t xgdb_workspace_bytes(const XgDims *d, int32_t S, int32_t Gd, int32_t Wg);

/*
 * Diverse beam search per pair.  Every group is the search of xgate_beam_control.h at W = Wg (its steps 1-5), with its own running
 * sums, its own done list of Wg entries and its own ranking.  Within step t the groups of a pair are merged in the order
 * j = 0 .. Gd-1, with one change to step 3:
 *   n_j(v) = the number of new slots of groups 0 .. j-1 at step t that are LIVE (their new sum p > -500) and hold word v.  Word 0
 *            counts like any other; dead slots never count.
 *   a[q][v] = lp[q][v] - lambda * n_j(v) for every row q of group j: in fp32 one multiply ((float)n * lambda) and one subtraction,
 *            each rounded on its own (no FMA).  lp carries the -1000 of suppress_token.
 *   Step 3 runs over a: row q contributes its Wg best a, lower word first on exact ties; candidate c_rank * rows + q carries
 *   p = sum[q] + a (one fp32 add); the first Wg of the stable descending sort are the group's new slots.  At t = 0 a group has one
 *   row, j * Wg, so at lambda > 0 the groups already open with different words.
 * sum = p carries the penalties; the r stored for the word is the UNPENALISED lp.  A beam's score is its penalised sum at the
 * moment it finished (what its group ranked by); seq_logp summed gives the pure sum.  Steps 4-5 per group are unchanged.
 * Gd = 1 is the plain rows-per-video search at W = Wg bit for bit, whatever lambda; at lambda = 0 every group equals that search.
 *   x                     as in xgate_beam_control.h: the B videos ONCE, pos_feats (B*S,R), row b * S + s
 *   seq (B*S,Gd,Wg,L)     int64 out: a group's done beams, best first, zero after a beam's finish
 *   seq_logp (B*S,Gd,Wg,L) their unpenalised r, zero after the finish
 *   score (B*S,Gd,Wg)     their penalised p
 *   trace (B*S,L,N,2)     int32 (token, parent) of every slot and step; the parent is a slot index of the PAIR, 0 .. N-1, and lies
 *                         in the slot's own group (at t = 0 it is j * Wg); NULL: not stored
 * XG_EINVAL, before anything is enqueued: everything the search of xgate_beam_control.h refuses at W = Gd * Wg (Gd * Wg > V,
 * Gd * Wg > XGDB_MAX_BEAM, suppress_token >= V, S < 1, the run modes, null pointers, invalid dims, the workspace's alignment,
 * B * S * Gd * Wg beyond 2^20 rows), Gd < 1, Wg < 1, and a lambda that is negative, infinite or NaN.  XG_EWORKSPACE: ws_bytes
 * below xgdb_workspace_bytes(d, S, Gd, Wg).
 */
int xgdb_beam_search(void *stream, const XgDims *d, int32_t S, int32_t Gd, int32_t Wg, float lambda, int32_t suppress_token,
                     const XgParams *p, const XgBnState *bn, const XgBatch *x, const XgRun *run, int64_t *seq, float *seq_logp,
                     float *score, int32_t *trace, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_BEAM_DIVERSE_H */
