/*
 * xgate_beam_rules.h -- C ABI of the CAPTIONER'S BEAM SEARCH UNDER DECODING RULES in libxgate_hip.so (gfx950): the search of
 * xgate_beam_allow.h -- the W best captions of each of B videos under each of its S `pos_feats` rows, on one shared encoder pass,
 * optionally with every step's words held to a POS template -- with four more controls: no repeated n-gram, a minimum length, no
 * end token right behind a listed word, and a length-scaled final ranking.
 *
 * Eval mode, fp32.  The conventions are those of xgate.h, xgate_beam.h, xgate_beam_control.h and xgate_beam_allow.h: device
 * pointers, caller-owned memory, every entry point only ENQUEUES work on `stream`, arguments are checked before anything is
 * enqueued, and a call does not depend on what the workspace held before.  d->B counts VIDEOS, d->T = seq_length + 1 = L + 1.  A
 * GROUP is one (video b, template s) pair, g = b * S + s, G = B * S groups; one row is one (group, slot) pair with row index
 * (b * S + s) * W + slot.  The encoder, init_hidden and v2a(V) run once on the B videos; no step needs the host.
 */
#ifndef XGATE_BEAM_RULES_H
#define XGATE_BEAM_RULES_H

#include "xgate_beam_allow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGBR_VERSION 1
#define XGBR_MAX_BAD_END 32
#define XGBR_MAX_LENGTH 512       /* the longest caption (L) the search serves: a row's history and ban list live in LDS */

typedef struct {
    int32_t no_repeat_ngram;      /* n >= 1: a live beam never holds the same n-gram twice; 0: off */
    int32_t min_length;           /* word 0 is banned at steps t < min_length; 0: off; at most L */
    const int32_t *bad_end;       /* device, n_bad_end words (each in [0, V)): word 0 is banned at a step t >= 1
                                     whose row's last word is one of them */
    int32_t n_bad_end;            /* 0 .. XGBR_MAX_BAD_END (32) */
    const float *length_scale;    /* device (L) or NULL (= all ones): every entry finite, in (0, 1] */
} XgBeamRules;

int xgbr_version(void);
/* bytes of the workspace of xgbr_beam_search at dims d (d->B = VIDEOS) with S templates per video and beam width W, whatever the
 * rules: what the search of xgate_beam_allow.h takes at the same d, S and W, plus two blocks of per-row histories (M,L) int32 and
 * the done list's keys (M); 0 for whatever that call refuses with XG_EINVAL on account of d, S and W, and for L above
 * XGBR_MAX_LENGTH */
size_t xgbr_workspace_bytes(const XgDims *d, int32_t S, int32_t W);

/*
 * The search is the rule of xgate_beam_allow.h, steps 1-5, per group, with these changes.
 *
 * History.  The history of row (group g, slot q) at step t is h[0..t-1]: the tokens of steps 0 .. t-1 of the slot it continues
 * (step 4 hands a new slot its parent's history with the new token appended).  BOS is not part of it.  Dead slots keep running and
 * keep a history like any other.
 *
 * The banned set Ban(row, t) is the union of three parts, and it is a SET: a word named twice is in it once.
 *   - with no_repeat_ngram = n >= 1: every word h[i+n-1] with 0 <= i <= t-n and h[i..i+n-2] == h[t-n+1..t-1] (the word that
 *     completed an earlier occurrence of the row's last n-1 words).  n = 1: every word of the history.  Empty while t < n.
 *   - word 0 when t < min_length.
 *   - word 0 when t >= 1 and h[t-1] is one of the n_bad_end words of bad_end.
 *
 * Step 2, the value of a word.  With `allow`, lp is what xgate_beam_allow.h gives (the log-softmax over the row's allowed words);
 * without it (word_cat and allow both NULL) lp is the row's plain log-softmax, as in xgate_beam_control.h.  A ban never changes the
 * log-sum-exp: seq_logp stays a log-probability of the model.  Then, in this order, each ONE fp32 subtraction rounded on its own:
 * 1000 off a word that is not allowed, 1000 off the suppressed word, 1000 off a word in Ban.  A banned word is thus what the
 * suppressed word is: a well-ordered candidate far below every live one.  A row still yields W distinct words; a slot that had to
 * take a banned word is dead (its sum is below -500).  Ties go to the lower word index, as everywhere.
 *
 * Step 5, the done list, is ordered by KEY, not by score.  A beam that finishes at step t with sum p has
 *     key = p * length_scale[t]   (one fp32 multiply)   if p > -500,        key = p   otherwise,
 * the list is kept stable and descending by key, a new entry behind entries of equal key; `score` still returns p and `key` the
 * key.  With every scale in (0, 1] a live entry has key > -500 >= every dead entry's key: length normalisation never lifts a dead
 * beam over a live one.  t = L-1 still finishes every slot, whatever its token.  length_scale NULL: key == score.
 *
 * What follows.
 *   - No returned beam with score > -500 holds the same n-gram twice among its words (the tokens before its first 0).
 *   - Every returned beam with score > -500 that ends with word 0 before step L-1 has at least min_length words, and its last word
 *     is not in bad_end.
 *   - With no_repeat_ngram = 0, min_length = 0, n_bad_end = 0 and length_scale NULL the launches produce what the search of
 *     xgate_beam_allow.h produces when `allow` is given, and what the search of xgate_beam_control.h produces when it is NULL: bit
 *     for bit in seq, seq_logp, score and trace, and key == score.
 *
 *   word_cat (V), allow (G,L)   as in xgate_beam_allow.h; BOTH NULL: no template constraint
 *   x                     feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- the B videos ONCE; pos_feats (B*S,R), row
 *                         b * S + s; seq / seq_mask are not read
 *   seq (G,W,L)           int64 out: a done beam's tokens, zero after its finish
 *   seq_logp (G,W,L)      its r (every -1000 included), zero after its finish
 *   score (G,W)           its p
 *   key (G,W)             its key; NULL: not stored
 *   trace (G,L,W,2)       int32 (token, parent slot) of every slot and step; NULL: not stored
 *
 * XG_EINVAL, before anything is enqueued: everything the searches of xgate_beam_allow.h / xgate_beam_control.h refuse, in their
 * order (S < 1 first); then L > XGBR_MAX_LENGTH; a NULL `rules`; no_repeat_ngram < 0 or > L; min_length < 0 or > L; n_bad_end < 0
 * or > XGBR_MAX_BAD_END; n_bad_end > 0 with a NULL bad_end; exactly one of word_cat / allow NULL.  XG_EWORKSPACE: ws_bytes below
 * xgbr_workspace_bytes(d, S, W).
 *
 * NOT checked: the contents of device tables cannot be read before the enqueue.  That every bad_end word lies in [0, V) and every
 * length_scale entry is finite and in (0, 1] is the CALLER'S duty.  The kernel clamps every word index it reads from a table (the
 * histories and bad_end) into [0, V), so a bad table can never index out of range; a scale outside (0, 1] merely voids the
 * live-before-dead guarantee above.
 */
int xgbr_beam_search(void *stream, const XgDims *d, int32_t S, int32_t W, int32_t suppress_token, const XgBeamRules *rules,
                     const uint8_t *word_cat, const uint32_t *allow, const XgParams *p, const XgBnState *bn, const XgBatch *x,
                     const XgRun *run, int64_t *seq, float *seq_logp, float *score, float *key, int32_t *trace, void *ws,
                     size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_BEAM_RULES_H */
