"""Test helper: the truncated (top-k / nucleus) caption draw of docs/CAPTION_TRUNCATED.md in numpy float64, and the rollout that
uses it, built from the oracle's own encoder, init_hidden, core_step and vocabulary product on the batch in which every video is
repeated S times.  Also the cases and settings that tests/test_cap_trunc_cpu.py (the cap condition) and
tests/test_gpu_cap_trunc.py (the kernel) share, so that the two files cannot drift apart.

`dtype` is the arithmetic of the MODEL (encoder, decoder steps, logits).  The selection itself -- sort, cumulative sums, whole
value classes -- always runs in float64 on those logits: it is the definition, not an implementation."""
import collections
import functools

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG

# (temperature, top_k, top_p)
SETTINGS = [(1.0, 0, 0.9), (1.0, 10, 1.0), (0.7, 8, 0.8), (1.0, 1, 1.0), (1.3, 0, 0.5)]
PEAK_GAIN = 10.0                      # `peaked`: logit.weight times this (chosen on the CPU: test_cap_trunc_cpu pins the nucleus size)
BIG_V = 40000                         # V * 4 bytes > 150 KB: the row is not staged in LDS
HUGE_V = 66000                        # more than 64 columns per thread: the search's per-thread bit set does not cover the row

# name -> (dims, S, gain of logit.weight)
CASES = {
    "tiny_s5": (CFG["tiny"], 5, 1.0),                            # V = 61 < threads, the generic step, logits from xgk_linear
    "mid_b3_s5": (dict(CFG["mid"], B=3), 5, 1.0),                # V = 500: the packed step, 32-column tile statistics
    "odd_s2": (CFG["odd"], 2, 1.0),                              # V = 37, V % 4 != 0
    "c1_s8": (dict(CFG["c1"], B=2, L=8), 8, 1.0),                # V = 20000: the staged row, 80-column statistics
    "rows_297": (dict(CFG["tiny"], B=9), 33, 1.0),               # more than 256 rows
    "big_v": (dict(CFG["tiny"], B=2, V=BIG_V), 3, 1.0),          # the global-memory form
    "huge_v": (dict(CFG["tiny"], B=2, V=HUGE_V), 2, 1.0),        # ... and the columns behind the bit set
    "peaked": (dict(CFG["mid"], B=3), 5, PEAK_GAIN),             # a nucleus of a few dozen words
}
# the settings each case runs: all of them where the issue's own check ran (and on `peaked`), a subset on the large ones
FIT = {name: list(SETTINGS) for name in ("tiny_s5", "mid_b3_s5", "odd_s2", "c1_s8", "peaked")}
FIT["rows_297"] = [SETTINGS[0], SETTINGS[2]]
FIT["big_v"] = [SETTINGS[0], SETTINGS[1], SETTINGS[2]]
FIT["huge_v"] = [SETTINGS[0], SETTINGS[2]]
PAIRS = [(name, s) for name in CASES for s in FIT[name]]

Kept = collections.namedtuple("Kept", "mask thr tau_k z_k need mass_at mass_above below")


def kept_set(x, temperature=1.0, top_k=0, top_p=1.0):
    """The kept set of one row of raw logits `x` (V), float64.  -> Kept: mask (V) bool; thr, the threshold value (K = {x >= thr});
    tau_k; z_k; need = top_p z_k; mass_at = mass{x >= thr} and mass_above = mass{x > thr}; below = the largest value under thr
    (-inf when there is none)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    w = np.exp((x - x.max()) / temperature)
    vals, inv = np.unique(x, return_inverse=True)                 # ascending; np.unique puts -0.0 and +0.0 in one class
    cls_mass = np.bincount(inv, weights=w, minlength=vals.size)[::-1]          # descending by value
    vals = vals[::-1]
    cum = np.cumsum(cls_mass)                                     # cum[i] = mass{x >= vals[i]}
    if top_k <= 0 or top_k >= V:
        ik = vals.size - 1
    else:
        tau = np.sort(x)[::-1][top_k - 1]                         # the k-th largest, counting multiplicity
        ik = int(np.flatnonzero(vals == tau)[0])
    z_k = float(cum[ik])
    need = float(top_p) * z_k
    ip = ik
    if top_p < 1.0:
        ip = min(int(np.flatnonzero(cum >= need)[0]), ik)        # the largest value whose upper set reaches the mass
    thr = float(vals[ip])
    return Kept(x >= thr, thr, float(vals[ik]), z_k, need, float(cum[ip]), float(cum[ip - 1]) if ip > 0 else 0.0,
                float(vals[ip + 1]) if ip + 1 < vals.size else -np.inf)


def draw(x, u, temperature=1.0, top_k=0, top_p=1.0):
    """One draw from a row.  -> (token, logp, logq, |K|, Kept, (lo, hi) the token's interval of the truncated CDF in [0, 1])"""
    x = np.asarray(x, dtype=np.float64)
    k = kept_set(x, temperature, top_k, top_p)
    mx = x.max()
    w = np.exp((x - mx) / temperature) * k.mask
    cdf = np.cumsum(w)
    tok = int(np.searchsorted(cdf, float(u) * cdf[-1], side="right"))
    if tok >= x.shape[0]:
        tok = int(np.flatnonzero(k.mask)[-1])
    lse = mx + np.log(np.exp(x - mx).sum())
    lo = (cdf[tok - 1] if tok > 0 else 0.0) / cdf[-1]
    return tok, float(x[tok] - lse), float(np.log(w[tok] / cdf[-1])), int(k.mask.sum()), k, (float(lo), float(cdf[tok] / cdf[-1]))


Ctx = collections.namedtuple("Ctx", "P V vproj state pos L dtype")


def prepare(P, x, pos, S, L, dtype=torch.float64):
    """The part of a rollout that no setting changes: encoder, initial state and v2a(V) of the batch with every video repeated S
    times.  P, x: numpy (paramgen); pos (B*S,R)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        Pt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in P.items()}
        rep = lambda k: torch.from_numpy(np.repeat(x[k], S, 0)).to(dtype)       # noqa: E731
        d = collections.namedtuple("D", "R")(Pt["logit.weight"].shape[1])
        with torch.no_grad():
            V = xo.encoder_fwd(Pt, rep("feats_rgb"), rep("feats_opfl"), rep("feat_mask"), train=False, running=xo.new_running(d))
            state = xo.init_hidden(Pt, V, rep("feat_mask"))
            vproj = xo._lin(V, Pt, "lstmcore.v2a")
    finally:
        torch.set_default_dtype(old)
    return Ctx(Pt, V, vproj, state, torch.from_numpy(pos).to(dtype), L, dtype)


def rollout(ctx, uniforms, temperature=1.0, top_k=0, top_p=1.0):
    """The rollout under the truncated draw, bookkeeping as xo.sample.  -> dict: seq (M,n) int64, seq_logp, seq_logq (M,n) float64,
    kept (M,n) int64 (seq_logq and kept 0 behind a row's end token), logits: per step t the (M,V) float64 raw logits the draw of
    step t + 1 read, and n."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(ctx.dtype)
    try:
        M = ctx.V.shape[0]
        state, unfinished = ctx.state, None
        seqs, lps, lqs, kepts, logits = [], [], [], [], []
        x = None
        with torch.no_grad():
            for t in range(ctx.L + 1):
                if t == 0:
                    it = torch.zeros(M, dtype=torch.int64)
                else:
                    rows = [draw(x[b], uniforms[t, b], temperature, top_k, top_p) for b in range(M)]
                    it = torch.tensor([r[0] for r in rows], dtype=torch.int64)
                    live = np.ones(M, bool) if unfinished is None else unfinished.numpy().copy()
                    unfinished = (it > 0) if t == 1 else unfinished & (it > 0)
                    if int(unfinished.sum()) == 0:
                        break
                    seqs.append((it * unfinished.to(it.dtype)).numpy())
                    lps.append(np.array([r[1] for r in rows]))
                    lqs.append(np.array([r[2] for r in rows]) * live)
                    kepts.append(np.array([r[3] for r in rows], dtype=np.int64) * live)
                mk = torch.ones(M, 1) if t == 0 else unfinished.to(ctx.dtype).unsqueeze(1)
                out, state, _ = xo.core_step(ctx.P, ctx.P["embed.weight"][it], mk, ctx.V, ctx.pos, state, t=t, train=False, vproj=ctx.vproj)
                x = xo._lin(out, ctx.P, "logit").double().numpy()
                logits.append(x)
    finally:
        torch.set_default_dtype(old)
    n = len(seqs)
    st = lambda a, dt: np.stack(a, 1) if n else np.zeros((M, 0), dt)            # noqa: E731
    return dict(seq=st(seqs, np.int64), seq_logp=st(lps, np.float64), seq_logq=st(lqs, np.float64), kept=st(kepts, np.int64),
                logits=logits, n=n)


# ---- the shared cases: inputs, uniforms and oracles, computed once and never changed
@functools.lru_cache(maxsize=None)
def params(name):
    dd, _, gain = CASES[name]
    P = dict(pg.make_params(pg.make_dims(**dd)._replace(B=1)))   # (the weights do not depend on B)
    if gain != 1.0:
        P["logit.weight"] = P["logit.weight"] * np.float32(gain)
    return P


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (dims, S, P, x, pos (B*S,R), uniforms (L+1, B*S))"""
    dd, S, _ = CASES[name]
    d = pg.make_dims(**dd)
    seed = 40 + len(name)
    x = pg.make_inputs(d, seed=seed, ragged=True)
    pos = pg.uniform("pos_feats_s", (d.B * S, d.R), seed, -1.0, 1.0)
    return d, S, params(name), x, pos, pg.uniform("u", (d.L + 1, d.B * S), seed)


@functools.lru_cache(maxsize=None)
def context(name, dtype=torch.float64):
    d, S, P, x, pos, _ = inputs(name)
    torch.set_num_threads(8)
    return prepare(P, x, pos, S, d.L, dtype)


@functools.lru_cache(maxsize=None)
def oracle(name, setting, dtype=torch.float64):
    T, k, p = setting
    return rollout(context(name, dtype), inputs(name)[5], T, k, p)


def first_differences(a, b):
    """Rows of two (M,n) / (M,n') integer arrays that differ -> {row: first differing column}, the shorter one padded with 0."""
    n = max(a.shape[1], b.shape[1])
    pad = lambda v: np.concatenate([v, np.zeros((v.shape[0], n - v.shape[1]), v.dtype)], 1)      # noqa: E731
    a, b = pad(np.asarray(a)), pad(np.asarray(b))
    return {int(r): int(np.flatnonzero(a[r] != b[r])[0]) for r in np.flatnonzero((a != b).any(1))}
