"""TEST INFRASTRUCTURE ONLY -- the captioner's beam search whose words must follow a POS template (include/xgate_beam_allow.h),
restated on top of tests/cap_beam_oracle.py: its rows (`_Rows`: the decoder step of oracle/xgate_oracle.py on the REPEATED batch),
the merge of tests/pos_beam_oracle.py (VideoSearch: steps 3-5) and, between the two, step 2 of the new header -- `constrain`.  It
runs on the CPU in the dtype it is asked for; float64 is the high-precision reference of tests/test_gpu_cap_allow.py.

`check_admissible` IS tests/pos_beam_oracle.check_admissible (every rule, LP_TOL = 3e-4, no row excused) over the constrained
float64 log-probabilities along the kernel's own trace: the words that are not allowed arrive there already lowered by 1000, exactly
as the suppressed word is lowered inside it.

The case table (CASES) and its inputs live here so that the CPU file can check the preconditions of the GPU file's cases."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import paramgen as pg
from tests import cap_beam_oracle as cbo
from tests import pos_beam_oracle as pbo
from tests.util import CFG

LP_TOL, LIVE, MARGIN = cbo.LP_TOL, cbo.LIVE, cbo.MARGIN
ANY = 0xFFFFFFFF


# ---- step 2 of include/xgate_beam_allow.h
def allowed_words(word_cat, allow):
    """(.., V) bool for masks (..) and the table (V,): word v is allowed iff bit (word_cat[v] & 31) of the mask; a mask that admits
    no word of the table counts as all ones."""
    cat = (np.asarray(word_cat).astype(np.int64) & 31)
    ok = ((np.asarray(allow).astype(np.int64)[..., None] >> cat) & 1).astype(bool)
    ok[~ok.any(-1)] = True
    return ok


def constrain(lp, ok):
    """lp (.., V): a row's log-softmax; ok (.., V) bool.  Returns lp - lse_a, lse_a the log-sum-exp of lp over the allowed words
    (the log-softmax of the logits over the allowed words wherever v is allowed), less 1000 at every word that is not allowed.  A row
    in which every word is allowed is returned as it is: its lse_a is the 0 that log_softmax already subtracted."""
    lp = np.array(lp)
    ok = np.broadcast_to(ok, lp.shape)
    part = ~ok.all(-1)
    if part.any():
        rows, oks = lp[part], ok[part]
        masked = np.where(oks, rows, -np.inf)
        mx = masked.max(-1, keepdims=True)
        lse = mx + np.log(np.exp(masked - mx).sum(-1, keepdims=True))
        lp[part] = (rows - lse - np.where(oks, 0, 1000)).astype(lp.dtype)
    return lp


def _group_masks(allow, G, L):
    a = np.asarray(allow).astype(np.int64)
    assert a.size == G * L, (a.shape, G, L)
    return a.reshape(G, L)


@torch.no_grad()
def allowed_beam_captions(Pn, xn, L, S, W, word_cat, allow, suppress_token=1, dtype=torch.float32):
    """The constrained search in `dtype` on the repeated batch `xn` (G = B S rows, tests/test_gpu_cap_beam_control.repeated) with
    the masks allow (B,S,L) or (G,L).  Returns what cap_beam_oracle.beam_captions returns, plus `logps` (G,L,W,V): every step's
    constrained log-probabilities before the suppressed word's -1000."""
    with cbo._default_dtype(dtype):
        P, x, running = cbo._cast(Pn, xn, dtype)
        rows = cbo._Rows(P, x, running, W)
        G = rows.B
        assert G % S == 0
        ok = allowed_words(word_cat, _group_masks(allow, G, L))                     # (G,L,V)
        vs, top_lp, top_ix, logps = None, [], [], []
        for t in range(L):
            lpn = constrain(rows.step().numpy(), ok[:, t, None, :])
            logps.append(lpn.copy())
            if vs is None:
                vs = [pbo.VideoSearch(W, L, lpn.dtype) for _ in range(G)]
            if suppress_token >= 0:
                lpn[:, :, suppress_token] -= 1000
            k = min(W + cbo.TOPK_EXTRA, lpn.shape[2])
            ix = np.argsort(-lpn, axis=2, kind="stable")[:, :, :k]
            top_ix.append(ix)
            top_lp.append(np.take_along_axis(lpn, ix, 2))
            par, nxt = zip(*[vs[g].feed(lpn[g]) for g in range(G)])
            rows.select(np.array(par), np.array(nxt))
    res = [v.result() for v in vs]
    trace = np.array([v.trace for v in vs])
    return dict(seq=np.array([[e["seq"] for e in r] for r in res]), seq_logp=np.array([[e["logps"] for e in r] for r in res]),
                score=np.array([[e["score"] for e in r] for r in res]), trace=trace, tokens=trace[..., 0].astype(np.int64),
                top_lp=np.stack(top_lp, 1), top_ix=np.stack(top_ix, 1).astype(np.int64), done=[v.done for v in vs], ranked=res,
                margin=np.array([v.margin for v in vs]), logps=np.stack(logps, 1))


def logps_along_trace(Pn, xn, trace, word_cat, allow, dtype=torch.float64):
    """cap_beam_oracle.logps_along_trace (G,L,W,V) with every row renormalised over its allowed words and the others lowered by
    1000 (`constrain`, the empty-set rule in `allowed_words`)."""
    lp = cbo.logps_along_trace(Pn, xn, trace, dtype)
    G, L = lp.shape[:2]
    return constrain(lp, allowed_words(word_cat, _group_masks(allow, G, L))[:, :, None, :])


def check_admissible(trace, r, score, seq, Pn, xn, L, W, word_cat, allow, suppress_token=1):
    """The kernel's own constrained search judged in float64 by tests/pos_beam_oracle.check_admissible (see there for every rule).
    Returns the number of (group, step) pairs checked."""
    return pbo.check_admissible(trace, r, score, seq, lambda tr: logps_along_trace(Pn, xn, tr, word_cat, allow, torch.float64),
                                C=Pn["logit.bias"].shape[0], L=L, W=W, suppress_tag=suppress_token)


# ---- tables and templates by seed
SINGLE, EMPTY, PAIR, NCAT = 2, 3, 4, 14     # the singleton category, the one no word has, the one of exactly two words; categories


def make_table(V, seed):
    """(V,) uint8: word 0 -> 0 and nothing else is 0, word 1 -> 1, one word of category SINGLE, none of EMPTY, two of PAIR (all
    three among the words from 2 on), the rest random over 1 and 5 .. NCAT-1."""
    assert V >= 5
    rng = np.random.RandomState(seed)
    rest = np.array([1] + list(range(5, NCAT)))
    t = rest[rng.randint(0, len(rest), V)].astype(np.uint8)
    pick = 2 + rng.permutation(V - 2)[:3]
    t[pick[0]], t[pick[1:]] = SINGLE, PAIR
    t[0], t[1] = 0, 1
    return t


def usable_tags(table):
    """The categories a template may name: non-zero, and held by at least one word that is not the suppressed word 1."""
    return sorted(set(int(c) for c in table[2:]))


KINDS = ("any", "two", "empty", "zero", "plain", "plain")        # group g is of kind KINDS[g % 6]


def make_constraints(G, L, table, seed):
    """Per group a ragged template of n single usable tags (1 <= n < L; n = 1 at L = 1) followed by tag 0, as masks (G,L) int64, and
    (tags (G,L) with -1 where a position is no single tag, n (G,), kinds).  Plain groups keep their template -- every third of them
    gets SINGLE at one position, every third PAIR --; in the others ONE position < n becomes 0xFFFFFFFF ("any"), two usable
    categories ("two"), the EMPTY category's bit ("empty": the fallback) or 0 ("zero": the fallback)."""
    rng = np.random.RandomState(seed)
    use = usable_tags(table)
    assert SINGLE in use and PAIR in use and EMPTY not in use and 0 not in use
    tags = np.zeros((G, L), np.int64)
    n = np.zeros(G, np.int64)
    kinds, plain = [], 0
    for g in range(G):
        n[g] = 1 if L == 1 else rng.randint(1, L)
        tags[g, :n[g]] = [use[i] for i in rng.randint(0, len(use), n[g])]
        kinds.append(KINDS[g % len(KINDS)])
    masks = np.left_shift(1, tags)
    for g in range(G):
        at = rng.randint(0, n[g])
        if kinds[g] == "plain":
            if plain % 3 < 2:
                tags[g, at] = (SINGLE, PAIR)[plain % 3]
                masks[g, at] = 1 << tags[g, at]
            plain += 1
            continue
        a, b = (use[i] for i in rng.permutation(len(use))[:2])
        masks[g, at] = {"any": ANY, "two": (1 << a) | (1 << b), "empty": 1 << EMPTY, "zero": 0}[kinds[g]]
        tags[g, at] = -1
    return masks, tags, n, kinds


# ---- the cases of tests/test_gpu_cap_allow.py: name -> (dims, S, W, input seed, logit_gain, table seed)
ALLOW_CFG = {"tiny": CFG["tiny"], "mid": CFG["mid"], "odd": CFG["odd"], "one": CFG["one"],
             "v20001": dict(CFG["tiny"], B=2, V=20001), "v38500": dict(CFG["tiny"], B=2, V=38500), "c1": dict(CFG["c1"], B=2)}
CASES = {
    "tiny_s3w3": ("tiny", 3, 3, 1, 32.0, 5),          # W = 3 above the PAIR category's two words
    "tiny_s5w1": ("tiny", 5, 1, 1, 32.0, 6),          # the greedy case
    "mid_s4w5": ("mid", 4, 5, 2, 128.0, 7),           # the packed step, 240 rows
    "odd_s2w2": ("odd", 2, 2, 3, 8.0, 8),             # V = 37, unaligned rows, the generic step
    "one_s6w2": ("one", 6, 2, 4, 8.0, 9),             # L = 1, V = 5: one group of every kind
    "v20001": ("v20001", 3, 3, 5, 8.0, 10),           # 80 KB of LDS, V % 4 = 1
    "v38500": ("v38500", 3, 3, 6, 8.0, 11),           # the unstaged form
    "c1_s2w5": ("c1", 2, 5, 7, 8.0, 12),              # the real layer sizes; every group of another special kind
}
PINNED = ("tiny_s3w3", "mid_s4w5")                    # seed and gain chosen on the CPU: tests/test_cap_allow_cpu.py has the counts


def make_pos(d, S, seed):
    """(B,S,R) float32: S different POS vectors per video (as tests/test_gpu_cap_beam_control.make_pos)."""
    return np.stack([pg.make_inputs(d, seed=seed + 101 * (s + 1))["pos_feats"] for s in range(S)], 1)


def repeated(x, pos):
    """The numpy batch in which video b is repeated S times, with pos_feats row b S + s."""
    S = pos.shape[1]
    xr = {k: np.repeat(v, S, 0) for k, v in x.items()}
    xr["pos_feats"] = np.ascontiguousarray(pos.reshape(-1, pos.shape[2]))
    return xr


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's fixed inputs: dict(d, P, x, pos (B,S,R), xr (the repeated batch), S, W, table (V,) uint8, masks (G,L) int64, tags, n,
    kinds).  Computed once and shared: nobody writes into it."""
    cfg, S, W, seed, gain, tseed = CASES[name]
    d = pg.make_dims(**ALLOW_CFG[cfg])
    P, x = pg.make_params(d, logit_gain=gain), pg.make_inputs(d, seed=seed, ragged=d.B >= 3)
    pos = make_pos(d, S, seed)
    table = make_table(d.V, tseed)
    masks, tags, n, kinds = make_constraints(d.B * S, d.L, table, tseed + 100)
    return dict(d=d, P=P, x=x, pos=pos, xr=repeated(x, pos), S=S, W=W, table=table, masks=masks, tags=tags, n=n, kinds=kinds)


SHORT_ROW = ("tiny", 3, 3, 4, 32.0, 5)                # a CASES entry for short_row_case: seed and gain chosen on the CPU as well


@functools.lru_cache(maxsize=None)
def short_row_case():
    """tiny at S = 3, W = 3 with the two-word category at position 0 of EVERY group and any word after it: at t = 0 the one row of
    a group yields the two words and, third, a word that carries the -1000.  A dict as `case` returns, plus `oracle`: its float64
    search."""
    cfg, S, W, seed, gain, tseed = SHORT_ROW
    d = pg.make_dims(**ALLOW_CFG[cfg])
    P, x = pg.make_params(d, logit_gain=gain), pg.make_inputs(d, seed=seed, ragged=True)
    pos = make_pos(d, S, seed)
    table = make_table(d.V, tseed)
    masks = np.full((d.B * S, d.L), ANY, np.int64)
    masks[:, 0] = 1 << PAIR
    c = dict(d=d, P=P, x=x, pos=pos, xr=repeated(x, pos), S=S, W=W, table=table, masks=masks)
    torch.set_num_threads(8)
    c["oracle"] = allowed_beam_captions(P, c["xr"], d.L, S, W, table, masks, dtype=torch.float64)
    return c


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """The float64 constrained search of a case (allowed_beam_captions), computed once."""
    c = case(name)
    torch.set_num_threads(8)
    return allowed_beam_captions(c["P"], c["xr"], c["d"].L, c["S"], c["W"], c["table"], c["masks"], dtype=torch.float64)
