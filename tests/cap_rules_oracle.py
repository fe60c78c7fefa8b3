"""TEST INFRASTRUCTURE ONLY -- the captioner's beam search under decoding rules (include/xgate_beam_rules.h), restated on top of
tests/cap_allow_oracle.py and tests/cap_beam_oracle.py: their rows (the decoder step of oracle/xgate_oracle.py on the REPEATED
batch), step 2 of xgate_beam_allow.h where masks are given, the merge of tests/pos_beam_oracle.py (VideoSearch) -- and the new
parts: `ban_sets` (the banned set of a row from its history), the histories carried along the parents, and the done list ordered by
key (`RuledSearch`).  It runs on the CPU in the dtype it is asked for; float64 is the reference of tests/test_gpu_cap_rules.py.

`check_admissible` is tests/pos_beam_oracle.check_admissible's rules (LP_TOL = 3e-4, eps_t = 2 (t + 1) 3e-4, no row excused) with
the done list judged by KEY: the existing function ranks the returned beams by score, so the variant is written here.

The case table (CASES), its inputs and the pinned counts (PINS: counted in float64 by tests/test_cap_rules_cpu.py) live here so
that the CPU file can check the preconditions of the GPU file's cases."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import paramgen as pg
from tests import cap_allow_oracle as cao
from tests import cap_beam_oracle as cbo
from tests import pos_beam_oracle as pbo
from tests import util
from tests.util import CFG

LP_TOL, LIVE, MARGIN, ANY = cbo.LP_TOL, cbo.LIVE, cbo.MARGIN, cao.ANY
OFF = dict(n=0, min_length=0, bad_end=(), scale=None)


def rules(n=0, min_length=0, bad_end=(), scale=None):
    """The rules as the oracle takes them: scale an (L,) float32 array or None."""
    return dict(n=int(n), min_length=int(min_length), bad_end=tuple(int(w) for w in bad_end),
                scale=None if scale is None else np.asarray(scale, np.float32))


# ---- the banned set of include/xgate_beam_rules.h
def ban_sets(h, n=0, min_length=0, bad_end=()):
    """The banned set of a row at step t = len(h) from its history h (the tokens of steps 0 .. t-1): the words that would complete
    an n-gram the history holds (n >= 1; empty while t < n), word 0 while t < min_length, word 0 behind a word of bad_end."""
    h = [int(w) for w in h]
    t, ban = len(h), set()
    if n >= 1 and t >= n:
        last = h[t - n + 1:]
        for i in range(t - n + 1):
            if h[i:i + n - 1] == last:
                ban.add(h[i + n - 1])
    if t < min_length:
        ban.add(0)
    if t >= 1 and h[t - 1] in set(bad_end):
        ban.add(0)
    return ban


def ban_mask(hist, V, rl):
    """(G,W,V) bool for the histories hist (G,W,t)."""
    G, W, _ = hist.shape
    out = np.zeros((G, W, V), bool)
    for g in range(G):
        for q in range(W):
            for w in ban_sets(hist[g, q], rl["n"], rl["min_length"], rl["bad_end"]):
                out[g, q, w] = True
    return out


def key_of(p, t, scale):
    """The key of a beam that finished at step t with sum p, in p's own precision: one multiply for a live p."""
    if scale is None or not p > LIVE:
        return p
    return p * p.dtype.type(scale[t])


class RuledSearch(pbo.VideoSearch):
    """VideoSearch with the done list ordered by key (include/xgate_beam_rules.h, step 5); hist(): every slot's tokens so far."""

    def __init__(self, W, L, dtype, scale=None):
        super().__init__(W, L, dtype)
        self.scale = scale

    def feed(self, lp):
        seen = len(self.done)
        out = super().feed(lp)
        for e in self.done[seen:]:
            e["key"] = key_of(e["score"], e["t"], self.scale)
        return out

    def hist(self):
        return self.seq[:self.t].T.copy()                           # (W,t)

    def result(self):
        order = np.argsort(-np.array([e["key"] for e in self.done]), kind="stable")[:self.W]
        return [self.done[i] for i in order]


@torch.no_grad()
def ruled_beam_captions(Pn, xn, L, S, W, rl=OFF, word_cat=None, allow=None, suppress_token=1, dtype=torch.float32):
    """The search under rules `rl` in `dtype` on the repeated batch `xn` (G = B S rows); word_cat / allow as
    cap_allow_oracle.allowed_beam_captions takes them, or both None.  Returns what that function returns (`logps`: before the
    suppressed word's and the bans' -1000) plus key (G,W) and t_fin (G,W), the step each returned beam finished at."""
    with cbo._default_dtype(dtype):
        P, x, running = cbo._cast(Pn, xn, dtype)
        rows = cbo._Rows(P, x, running, W)
        G = rows.B
        assert G % S == 0 and (word_cat is None) == (allow is None)
        ok = None if allow is None else cao.allowed_words(word_cat, cao._group_masks(allow, G, L))
        vs, top_lp, top_ix, logps = None, [], [], []
        for t in range(L):
            lpn = rows.step().numpy()
            lpn = lpn.copy() if ok is None else cao.constrain(lpn, ok[:, t, None, :])
            logps.append(lpn.copy())
            if vs is None:
                vs = [RuledSearch(W, L, lpn.dtype, rl["scale"]) for _ in range(G)]
            if suppress_token >= 0:
                lpn[:, :, suppress_token] -= 1000
            lpn[ban_mask(np.stack([v.hist() for v in vs]), lpn.shape[2], rl)] -= 1000
            k = min(W + cbo.TOPK_EXTRA, lpn.shape[2])
            ix = np.argsort(-lpn, axis=2, kind="stable")[:, :, :k]
            top_ix.append(ix)
            top_lp.append(np.take_along_axis(lpn, ix, 2))
            par, nxt = zip(*[vs[g].feed(lpn[g]) for g in range(G)])
            rows.select(np.array(par), np.array(nxt))
    res = [v.result() for v in vs]
    trace = np.array([v.trace for v in vs])
    return dict(seq=np.array([[e["seq"] for e in r] for r in res]), seq_logp=np.array([[e["logps"] for e in r] for r in res]),
                score=np.array([[e["score"] for e in r] for r in res]), key=np.array([[e["key"] for e in r] for r in res]),
                t_fin=np.array([[e["t"] for e in r] for r in res]), trace=trace, tokens=trace[..., 0].astype(np.int64),
                top_lp=np.stack(top_lp, 1), top_ix=np.stack(top_ix, 1).astype(np.int64), done=[v.done for v in vs], ranked=res,
                margin=np.array([v.margin for v in vs]), logps=np.stack(logps, 1))


def histories_of(trace):
    """(G,L,W,L) int64 from a trace (G,L,W,2): [g,t,q,:t] is the history of row q at step t (zeros behind it)."""
    trace = np.asarray(trace)
    G, L, W, _ = trace.shape
    out = np.zeros((G, L, W, L), np.int64)
    cur = np.zeros((G, W, L), np.int64)
    gi = np.arange(G)[:, None]
    for t in range(L):
        out[:, t] = cur
        cur = cur[gi, trace[:, t, :, 1].astype(np.int64)]
        cur[:, :, t] = trace[:, t, :, 0]
    return out


def logps_along_trace(Pn, xn, trace, rl, word_cat=None, allow=None, dtype=torch.float64):
    """(G,L,W,V): the log-probabilities every step's merge sees along a given trace with every -1000 but the suppressed word's
    applied: the words that are not allowed (cap_allow_oracle.logps_along_trace) and the banned sets of the histories rebuilt from
    that trace."""
    lp = cbo.logps_along_trace(Pn, xn, trace, dtype) if allow is None else cao.logps_along_trace(Pn, xn, trace, word_cat, allow, dtype)
    lp = np.array(lp)
    hist = histories_of(trace)
    for t in range(lp.shape[1]):
        lp[:, t][ban_mask(hist[:, t, :, :t], lp.shape[3], rl)] -= 1000
    return lp


def check_admissible(trace, r, score, key, seq, Pn, xn, L, W, rl, word_cat=None, allow=None, suppress_token=1):
    """The kernel's own search under rules judged in float64: tests/pos_beam_oracle.check_admissible's rules for every live
    selection over `logps_along_trace`, then the returned beams with the done list judged by KEY: each is a distinct completion of
    the trace with its tokens verbatim, every r within 3e-4, its score within eps_t of the float64 one and its key within eps_t of
    the float64 key (a scale is at most 1); the returned keys descend, equal keys in completion order, and no completion left out
    has a float64 key above the worst returned one by more than 2 L 3e-4.  Returns the number of (group, step) pairs checked."""
    trace, r, score, key, seq = (np.asarray(a) for a in (trace, r, score, key, seq))
    Cn, sup, scale = Pn["logit.bias"].shape[0], suppress_token, rl["scale"]
    B = trace.shape[0]
    assert trace.shape == (B, L, W, 2) and r.shape == (B, W, L) and score.shape == (B, W) and key.shape == (B, W) and seq.shape == (B, W, L)
    cols = min(W, Cn)
    assert trace[..., 0].min() >= 0 and trace[..., 0].max() < Cn and trace[..., 1].min() >= 0 and trace[..., 1].max() < W
    assert (trace[:, 0, :, 1] == 0).all()
    lp_all = logps_along_trace(Pn, xn, trace, rl, word_cat, allow, torch.float64)
    assert lp_all.dtype == np.float64 and lp_all.shape == (B, L, W, Cn)
    sums, r64 = np.zeros((B, W)), np.zeros((B, L, W))
    events = [[] for _ in range(B)]                               # completion order: (t, slot, float64 score, float64 key)
    checked = 0
    for t in range(L):
        lp = lp_all[:, t].copy()
        if sup >= 0:
            lp[:, :, sup] -= 1000
        rows = 1 if t == 0 else W
        eps = 2 * (t + 1) * LP_TOL
        tk, par = trace[:, t, :, 0].astype(np.int64), trace[:, t, :, 1].astype(np.int64)
        ys = -np.sort(-lp[:, :rows], axis=2)[:, :, :cols]
        cand = (sums[:, :rows, None] + ys).reshape(B, -1)
        wth = -np.sort(-cand, axis=1)[:, W - 1]
        bi = np.arange(B)[:, None]
        rr = lp[bi, par, tk]
        p = sums[bi, par] + rr
        r64[:, t] = rr
        for b in range(B):
            if not (p[b] > LIVE).any():
                continue
            checked += 1
            where = "group %d step %d" % (b, t)
            assert (rr[b] >= ys[b, par[b], cols - 1] - LP_TOL).all(), (where, "a token outside its row's top", rr[b], ys[b])
            assert (p[b] >= wth[b] - eps).all(), (where, "a selected candidate below the W-th best", p[b], wth[b])
            assert (p[b, :-1] >= p[b, 1:] - eps).all(), (where, "slots out of order", p[b])
            assert len({(int(a), int(k)) for a, k in zip(par[b], tk[b])}) == W, (where, "a candidate taken twice")
        sums = p.copy()
        fin = (tk == 0) | (t == L - 1)
        for b, v in zip(*np.nonzero(fin)):
            events[b].append((t, int(v), p[b, v], key_of(np.float64(p[b, v]), t, scale)))
        sums[fin] = -1000
    for b in range(B):
        ev = events[b]
        assert len(ev) >= W
        beams = [pbo.backtrace(trace[b], t, v) for t, v, _, _ in ev]
        used = []
        for k in range(W):
            match = [i for i, (t, v, p64, k64) in enumerate(ev) if i not in used and np.array_equal(beams[i][0], seq[b, k]) and
                     abs(p64 - score[b, k]) <= 2 * (t + 1) * LP_TOL and abs(k64 - key[b, k]) <= 2 * (t + 1) * LP_TOL]
            assert match, ("group %d rank %d is no completion of the trace" % (b, k), seq[b, k], score[b, k], key[b, k], ev)
            i = match[0]
            used.append(i)
            t, v, p64, k64 = ev[i]
            path = r64[b, np.arange(t + 1), beams[i][1][:t + 1]]
            np.testing.assert_allclose(r[b, k, :t + 1], path, atol=LP_TOL, err_msg="group %d rank %d" % (b, k))
            assert (r[b, k, t + 1:] == 0).all() and (seq[b, k, t + 1:] == 0).all()
        assert (key[b, :-1] >= key[b, 1:]).all(), (b, key[b])
        for k in range(W - 1):
            if key[b, k] == key[b, k + 1]:
                assert used[k] < used[k + 1], (b, k, "equal keys out of completion order")
        worst = min(ev[i][3] for i in used)
        for i, (t, v, p64, k64) in enumerate(ev):
            if i not in used:
                assert k64 <= worst + 2 * L * LP_TOL, ("group %d: completion (%d,%d) left out" % (b, t, v), k64, worst)
    return checked


# ---- host-side predicates over returned beams
def words_of(seq):
    """The words of a caption: its tokens before the first 0."""
    seq = [int(w) for w in seq]
    return seq[:seq.index(0)] if 0 in seq else seq


def has_repeat(seq, n):
    w = words_of(seq)
    grams = [tuple(w[i:i + n]) for i in range(len(w) - n + 1)]
    return len(set(grams)) < len(grams)


# ---- the cases of tests/test_gpu_cap_rules.py
RULES_CFG = {"tiny12": dict(CFG["tiny"], L=12), "odd9": dict(CFG["odd"], L=9), "mid12": dict(CFG["mid"], L=12), "one": CFG["one"],
             "v20001": dict(CFG["tiny"], B=2, V=20001, L=8), "v38500": dict(CFG["tiny"], B=2, V=38500, L=8),
             "c1": dict(CFG["c1"], B=2)}
# name -> (dims, S, W, input seed, logit_gain (None: util.eos_params), n, min_length)
CASES = {
    "tiny_n1": ("tiny12", 3, 3, 1, 32.0, 1, 0),
    "tiny_n2": ("tiny12", 3, 3, 1, 32.0, 2, 0),
    "odd_n1": ("odd9", 2, 2, 3, 8.0, 1, 0),               # V = 37, unaligned rows, the generic step
    "mid_n3": ("mid12", 2, 5, 2, 128.0, 3, 0),            # the packed step
    "one_n1": ("one", 2, 2, 4, 8.0, 1, 0),                # L = 1, V = 5: no ban can fire
    "v20001_n2": ("v20001", 3, 3, 5, 8.0, 2, 0),          # 80 KB staged, V % 4 = 1
    "v38500_n2": ("v38500", 3, 3, 6, 8.0, 2, 0),          # the unstaged form
    "c1_n3": ("c1", 2, 5, 7, 8.0, 3, 0),                  # the real layer sizes
    "eos_min3": ("tiny12", 3, 3, 2, None, 0, 3),
    "eos_min3_n2": ("tiny12", 3, 3, 2, None, 2, 3),
    "mideos_min3": ("mid12", 2, 5, 2, None, 0, 3),
}
REPETITION = ("tiny_n1", "tiny_n2", "odd_n1", "mid_n3")   # seed and gain chosen on the CPU: every plain group repeats
LENGTH = ("eos_min3", "eos_min3_n2", "mideos_min3")
TRACE_CASES = ("tiny_n1", "tiny_n2", "odd_n1", "mid_n3", "one_n1", "v20001_n2", "v38500_n2", "c1_n3")
# Counted in float64 (tests/test_cap_rules_cpu.py::test_preconditions_of_the_gpu_cases asserts them):
#   groups: G;  plain_rep: groups whose PLAIN search has a live beam with a repeated n-gram;  ruled_rep: live ruled beams with one;
#   live_best: groups whose ruled search's best beam is live;  plain_short / ruled_short: groups whose best beam has fewer than
#   min_length words
PINS = {
    "tiny_n1": dict(groups=15, plain_rep=15, ruled_rep=0, live_best=15),
    "tiny_n2": dict(groups=15, plain_rep=15, ruled_rep=0, live_best=15),
    "odd_n1": dict(groups=6, plain_rep=6, ruled_rep=0, live_best=6),
    "mid_n3": dict(groups=24, plain_rep=24, ruled_rep=0, live_best=24),
    "eos_min3": dict(groups=15, plain_short=15, ruled_short=0, live_best=15),
    "eos_min3_n2": dict(groups=15, plain_short=15, ruled_short=0, live_best=15, ruled_rep=0),
    "mideos_min3": dict(groups=24, plain_short=24, ruled_short=0, live_best=24),
}
# the bad-endings case: eos_min3's inputs with min_length off; the list is the words the PLAIN float64 search's live beams end on
BAD_END_CASE = "eos_min3"
# the length-scale cases: eos_min3's inputs with min_length off, (alpha, kind)
SCALE_FORMS = {"avg1": (1.0, "avg"), "wu07": (0.7, "wu")}


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's fixed inputs: dict(d, P, x, pos (B,S,R), xr (the repeated batch), S, W, rl).  Computed once and shared: nobody
    writes into it."""
    cfg, S, W, seed, gain, n, mn = CASES[name]
    d = pg.make_dims(**RULES_CFG[cfg])
    P = util.eos_params(d) if gain is None else pg.make_params(d, logit_gain=gain)
    x = pg.make_inputs(d, seed=seed, ragged=d.B >= 3)
    pos = cao.make_pos(d, S, seed)
    return dict(d=d, P=P, x=x, pos=pos, xr=cao.repeated(x, pos), S=S, W=W, rl=rules(n=n, min_length=mn))


@functools.lru_cache(maxsize=None)
def oracle64(name, ruled=True):
    """The float64 search of a case, under its rules or (ruled=False) without any; computed once."""
    c = case(name)
    torch.set_num_threads(8)
    return ruled_beam_captions(c["P"], c["xr"], c["d"].L, c["S"], c["W"], c["rl"] if ruled else OFF, dtype=torch.float64)


def scale_table(L, form):
    from controllable_xgating_amd import length_scale_table
    alpha, kind = SCALE_FORMS[form]
    return length_scale_table(L, alpha, kind).numpy()


@functools.lru_cache(maxsize=None)
def scale_oracle64(form):
    c = case(BAD_END_CASE)
    torch.set_num_threads(8)
    return ruled_beam_captions(c["P"], c["xr"], c["d"].L, c["S"], c["W"], rules(scale=scale_table(c["d"].L, form)), dtype=torch.float64)


def live_endings(o):
    """The sorted words on which live returned beams of a search end with word 0 before step L-1 (the word before that 0)."""
    out = set()
    L = o["seq"].shape[2]
    for g, k in np.argwhere(o["score"] > LIVE):
        w = words_of(o["seq"][g, k])
        if w and o["t_fin"][g, k] < L - 1:
            out.add(w[-1])
    return sorted(out)


PINNED_BAD_END = (21, 37, 53)         # live_endings of BAD_END_CASE's plain float64 search
# groups (of 15) in which the float64 key order of the returned beams differs from their order by score
PINNED_REORDERED = {"avg1": 4, "wu07": 0}


def reordered_groups(o):
    W = o["score"].shape[1]
    return sum(not np.array_equal(np.argsort(-o["score"][g], kind="stable"), np.arange(W)) for g in range(o["score"].shape[0]))


def count_pins(name):
    """What PINS records for a case, counted on the float64 oracle."""
    c, o, pl = case(name), oracle64(name), oracle64(name, False)
    n, mn = c["rl"]["n"], c["rl"]["min_length"]
    G = c["d"].B * c["S"]
    out = dict(groups=G, live_best=int((o["score"][:, 0] > LIVE).sum()))
    if n:
        live = lambda r, g: [k for k in range(c["W"]) if r["score"][g, k] > LIVE]      # noqa: E731
        if name in REPETITION:
            out["plain_rep"] = sum(any(has_repeat(pl["seq"][g, k], n) for k in live(pl, g)) for g in range(G))
        out["ruled_rep"] = sum(has_repeat(o["seq"][g, k], n) for g in range(G) for k in live(o, g))
    if mn:
        out["plain_short"] = sum(len(words_of(pl["seq"][g, 0])) < mn for g in range(G))
        out["ruled_short"] = sum(len(words_of(o["seq"][g, 0])) < mn for g in range(G))
    return out
