"""TEST INFRASTRUCTURE ONLY -- the captioner's beam search (include/xgate_beam.h) restated on top of oracle/xgate_oracle.py
(encoder_fwd in eval mode, init_hidden, core_step, the logit head), with the merge of tests/pos_beam_oracle.py (VideoSearch /
merge_step: steps 3-5 are the same rules for both searches).  It runs on the CPU in the dtype it is asked for: float32 against the
fixtures tests/golden/cap_beam_*.npz, float64 as the high-precision reference of tests/test_gpu_cap_beam.py.

`check_admissible` judges a search the KERNEL made, where margins are too tight to pin its tokens.  It IS
tests/pos_beam_oracle.check_admissible -- the same code, the same LP_TOL = 3e-4 and eps_t = 2 (t + 1) 3e-4, every live selection
and every returned beam, no row excused -- run over the captioner's float64 log-probabilities along the kernel's own trace."""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import pos_beam_oracle as pbo
from tests import util

GOLD = pbo.GOLD
LP_TOL, LIVE, MARGIN = pbo.LP_TOL, pbo.LIVE, pbo.MARGIN
TOPK_EXTRA = 1                                # the fixtures keep the W + 1 largest log-probabilities of every step and slot
# fixture tests/golden/cap_beam_<name>.npz -> (util.CFG entry, B or None, eos_params scaling, input seed, W)
BEAM_CASES = {"tiny_w3": ("tiny", None, False, 0, 3), "eos_w3": ("tiny", None, True, 2, 3),
              "mideos_w5": ("mid", None, True, 2, 5), "c1_w5": ("c1", 3, False, 0, 5)}


def case_setup(name):
    """(d, P, x, W) of a fixture: numpy parameters and inputs."""
    cfg, B, eos, seed, W = BEAM_CASES[name]
    c = dict(util.CFG[cfg])
    if B is not None:
        c["B"] = B
    d = pg.make_dims(**c)
    return d, (util.eos_params(d) if eos else pg.make_params(d)), pg.make_inputs(d, seed=seed), W


def load_case(name):
    """(d, P, x, W, the fixture) of tests/golden/cap_beam_<name>.npz."""
    return case_setup(name) + (dict(np.load(os.path.join(GOLD, "cap_beam_%s.npz" % name))),)


@contextlib.contextmanager
def _default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _cast(Pn, xn, dtype):
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in Pn.items()}
    x = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in xo.to_torch_inputs(xn).items()}
    return P, x, xo.new_running(pg.make_dims(R=P["logit.weight"].shape[1]))       # (eval mode on fresh running statistics)


class _Rows:
    """The M = B W rows of a search: everything computed once per video and row-repeated, and the step on all rows."""

    def __init__(self, P, x, running, W):
        self.P, self.W = P, W
        V = xo.encoder_fwd(P, x["feats_rgb"], x["feats_opfl"], x["feat_mask"], train=False, running=running)
        state = xo.init_hidden(P, V, x["feat_mask"])
        vproj = xo._lin(V, P, "lstmcore.v2a")
        rep = lambda t: t.repeat_interleave(W, 0)                                     # noqa: E731
        self.V, self.vproj, self.pos = rep(V), rep(vproj), rep(x["pos_feats"])
        self.state = [tuple(rep(s) for s in layer) for layer in state]
        self.B, self.M = V.shape[0], V.shape[0] * W
        self.base = (torch.arange(self.B) * W).unsqueeze(1)
        self.one = torch.ones(self.M, 1)
        self.tok = torch.zeros(self.M, dtype=torch.int64)
        self.t = 0

    def step(self):
        """(B,W,V) log-probabilities of the fed tokens' step (before the -1000)."""
        out, self.state, _ = xo.core_step(self.P, self.P["embed.weight"][self.tok], self.one, self.V, self.pos, self.state,
                                          t=self.t, train=False, vproj=self.vproj)
        self.t += 1
        return torch.log_softmax(xo._lin(out, self.P, "logit"), dim=1).reshape(self.B, self.W, -1)

    def select(self, parents, tokens):
        """Slot v continues slot parents[b, v] and is fed tokens[b, v]."""
        rows = (torch.as_tensor(np.asarray(parents, np.int64)) + self.base).reshape(self.M)
        self.state = [tuple(s[rows] for s in layer) for layer in self.state]
        self.tok = torch.as_tensor(np.asarray(tokens, np.int64)).reshape(self.M)


@torch.no_grad()
def beam_captions(Pn, xn, L, W, suppress_token=1, dtype=torch.float32):
    """The search in `dtype`.  Returns a dict: seq (B,W,L) int64, seq_logp (B,W,L), score (B,W), trace (B,L,W,2) int32, tokens
    (B,L,W), top_lp / top_ix (B,L,W,W+1) -- every step's and slot's W + 1 largest log-probabilities after the -1000 --, done (per
    video, completion order), ranked, margin (B,)."""
    with _default_dtype(dtype):
        P, x, running = _cast(Pn, xn, dtype)
        rows = _Rows(P, x, running, W)
        B = rows.B
        vs, top_lp, top_ix = None, [], []
        for t in range(L):
            lpn = rows.step().numpy().copy()
            if vs is None:
                vs = [pbo.VideoSearch(W, L, lpn.dtype) for _ in range(B)]
            if suppress_token >= 0:
                lpn[:, :, suppress_token] -= 1000
            k = min(W + TOPK_EXTRA, lpn.shape[2])
            ix = np.argsort(-lpn, axis=2, kind="stable")[:, :, :k]
            top_ix.append(ix)
            top_lp.append(np.take_along_axis(lpn, ix, 2))
            par, nxt = zip(*[vs[b].feed(lpn[b]) for b in range(B)])
            rows.select(np.array(par), np.array(nxt))
    res = [v.result() for v in vs]
    trace = np.array([v.trace for v in vs])
    return dict(seq=np.array([[e["seq"] for e in r] for r in res]), seq_logp=np.array([[e["logps"] for e in r] for r in res]),
                score=np.array([[e["score"] for e in r] for r in res]), trace=trace, tokens=trace[..., 0].astype(np.int64),
                top_lp=np.stack(top_lp, 1), top_ix=np.stack(top_ix, 1).astype(np.int64), done=[v.done for v in vs], ranked=res,
                margin=np.array([v.margin for v in vs]))


@torch.no_grad()
def logps_along_trace(Pn, xn, trace, dtype=torch.float64):
    """(B,L,W,V) numpy: the log-probabilities (before the -1000) every step's merge sees when the states are teacher-forced along a
    given search: slot v of step t continues slot trace[b,t,v,1] and is fed the token trace[b,t,v,0]."""
    trace = np.asarray(trace)
    B, L, W, _ = trace.shape
    with _default_dtype(dtype):
        P, x, running = _cast(Pn, xn, dtype)
        rows = _Rows(P, x, running, W)
        out = []
        for t in range(L):
            out.append(rows.step().numpy())
            rows.select(trace[:, t, :, 1], trace[:, t, :, 0])
    return np.stack(out, 1)


def replay_fixture(g, W, L):
    """Steps 3-5 over a fixture's recorded W + 1 largest log-probabilities: per video the VideoSearch after L steps.  The
    merge only ever reads a row's W largest, so the sparse rows (everything else far below) give what the full rows gave."""
    B = g["top_lp"].shape[0]
    out = []
    for b in range(B):
        vs = pbo.VideoSearch(W, L, np.float32)
        for t in range(L):
            vs.feed(sparse_rows(g["top_lp"][b, t], g["top_ix"][b, t]))
        out.append(vs)
    return out


def sparse_rows(top_lp, top_ix):
    """(W,k) values and word indices -> (W, max index + 1) rows that hold them and -3000 elsewhere."""
    rows = np.full((top_lp.shape[0], int(top_ix.max()) + 1), -3000, np.float32)
    np.put_along_axis(rows, top_ix, top_lp.astype(np.float32), 1)
    return rows


def check_admissible(trace, r, score, seq, Pn, xn, L, W, suppress_token=1):
    """The kernel's own search, judged in float64 by tests/pos_beam_oracle.check_admissible (see there for every rule) over the
    captioner's log-probabilities along that trace.  trace (B,L,W,2), r = the returned seq_logp (B,W,L), score (B,W), seq (B,W,L)
    as numpy.  Returns the number of (video, step) pairs checked."""
    return pbo.check_admissible(trace, r, score, seq, lambda tr: logps_along_trace(Pn, xn, tr, torch.float64),
                                C=Pn["logit.bias"].shape[0], L=L, W=W, suppress_tag=suppress_token)
