/*
 * xgate_beam_allow.h -- C ABI of the CAPTIONER'S BEAM SEARCH WHOSE WORDS MUST FOLLOW A POS TEMPLATE in libxgate_hip.so (gfx950): the
 * search of xgate_beam_control.h -- the W most likely captions of each of B videos under each of its S `pos_feats` rows, on one
 * shared encoder pass -- in which, at step t of a group's captions, only words whose POS category the group admits at t take part in
 * the softmax, and every other word is treated like the suppressed one.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h, xgate_beam.h and xgate_beam_control.h: device pointers, caller-owned
 * memory, every entry point only ENQUEUES work on `stream`, arguments are checked before anything is enqueued, and a call does not
 * depend on what the workspace held before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1.  A GROUP is one (video b, template
 * s) pair, g = b * S + s, G = B * S groups; one row is one (group, slot) pair with row index (b * S + s) * W + slot.  The encoder,
 * init_hidden and v2a(V) run once on the B videos; no step needs the host.
 */
#ifndef XGATE_BEAM_ALLOW_H
#define XGATE_BEAM_ALLOW_H

#include "xgate_beam_control.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGBA_VERSION 1

int xgba_version(void);
/* bytes of the workspace of xgba_beam_search at dims d (d->B = VIDEOS) with S templates per video and beam width W: what the search
 * of xgate_beam_control.h takes at the same d, S and W (the predicate needs no table of its own); 0 for whatever that call refuses
 * with XG_EINVAL on account of d, S and W */
size_t xgba_workspace_bytes(const XgDims *d, int32_t S, int32_t W);

/*
 * The constraint.
 *   word_cat (V)          uint8: the category of every word of the vocabulary.  Values are below 32; the kernel reads
 *                         word_cat[v] & 31, so no shift is ever out of range.
 *   allow (G,L)           uint32: for group g and step t the bit set of admitted categories.  Word v is ALLOWED in group g at step
 *                         t iff (allow[g * L + t] >> (word_cat[v] & 31)) & 1.  A single tag c is 1u << c, "any word" is
 *                         0xFFFFFFFF, "noun or adjective" is two bits.  A set that admits NO word of the vocabulary -- a zero
 *                         mask included -- counts as 0xFFFFFFFF for that row and step: no softmax is ever empty.
 *
 * Beam search per group.  Every group runs on its own: W slots with running sums sum[W] = 0, all starting from its VIDEO's
 * init_hidden state, all gated by the group's pos_feats row.  For t = 0 .. L-1:
 *   1. the decoder step on every slot with mask 1, fed BOS (0) at t = 0 and the slot's token of step t - 1 after it.  Dead slots
 *      keep running.
 *   2. lse_a = the log-sum-exp of the slot's logits over its ALLOWED words only; lp[q][v] = logit(h2_q)[v] - lse_a for EVERY word
 *      (where v is allowed: the log-softmax of the logits with the other columns at -inf); then lp[q][v] -= 1000 for every word
 *      that is NOT allowed, and lp[q][suppress_token] -= 1000 when suppress_token >= 0 (any negative value turns it off).  A word
 *      that is not allowed is thus what the suppressed word is: a well-ordered candidate far below every live one, so a row whose
 *      allowed set is smaller than W still yields W distinct words, and a slot that had to take one is a dead slot (its sum is
 *      below -500).  At a step whose allowed set is a single word that word's lp is exactly 0.
 *   3. rows = 1 at t = 0, else W.  Per row the W largest lp in descending order, lower word index first on exact ties of the fp32
 *      lp; candidate c_rank * rows + q has p = sum[q] + lp (one fp32 add); a stable sort by p descending; the first W are the new
 *      slots 0 .. W-1.
 *   4. new slot v takes the whole state (h1, c1, h2, c2) of its parent slot q; its token is the candidate's word,
 *      r[t][v] = lp (every -1000 included), sum[v] = p.
 *   5. for v = 0 .. W-1 in order: a token 0, or t = L-1, appends the beam to the group's done list with score p and sets
 *      sum[v] = -1000.  The done beam holds its tokens and r for steps 0 .. t, zeros after.
 * The result per group is its done list stable-sorted by score descending, first W entries (at least W always exist): each beam
 * is ranked by its score AT THE MOMENT IT FINISHED.  Groups never interact.
 *
 * What follows: every token of a returned beam whose score is above -500 is allowed at its position; with a table in which word 0
 * is the only word of category 0 and a group's masks n < L single non-zero tags followed by tag 0, every such beam has exactly n
 * words and finishes at step n; with every mask 0xFFFFFFFF the search is that of xgate_beam_control.h.
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (B*S,R), row
 *                         b * S + s; seq / seq_mask are not read
 *   seq (G,W,L)           int64 out: a done beam's tokens, zero after its finish
 *   seq_logp (G,W,L)      its r, zero after its finish
 *   score (G,W)           its p
 *   trace (G,L,W,2)       int32 (token, parent slot) of every slot and step; NULL: not stored
 * XG_EINVAL, before anything is enqueued: S < 1; everything the search of xgate_beam.h refuses (W < 1, W > V, W above its widest
 * beam, 8, suppress_token >= V, run->train, run->save, a run->gemm_mode other than 0, a null pointer other than `trace` -- bn and
 * its four statistics included --, invalid dims, d->T < 2 among them, a workspace that is not 256-byte aligned) and B * S * W beyond
 * 2^20 rows, in the order of xgate_beam_control.h; then a null word_cat or allow.  XG_EWORKSPACE: ws_bytes below
 * xgba_workspace_bytes(d, S, W).
 */
int xgba_beam_search(void *stream, const XgDims *d, int32_t S, int32_t W, int32_t suppress_token, const uint8_t *word_cat,
                     const uint32_t *allow, const XgParams *p, const XgBnState *bn, const XgBatch *x, const XgRun *run,
                     int64_t *seq, float *seq_logp, float *score, int32_t *trace, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_BEAM_ALLOW_H */
