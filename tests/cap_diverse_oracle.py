"""TEST INFRASTRUCTURE ONLY -- the captioner's diverse beam search (include/xgate_beam_diverse.h) restated over
tests/cap_beam_oracle._Rows (the captioner's float32 / float64 step on the REPEATED batch: one entry of the batch per (video,
template) pair) with the group rule of tests/pos_diverse_oracle.PairSearch.  `check_admissible` judges a search the KERNEL made: it
IS tests/pos_diverse_oracle.check_admissible_groups -- the same LP_TOL = 3e-4 and eps_t = 2 (t + 1) 3e-4, every group, none
excused -- over the captioner's float64 log-probabilities along the kernel's own trace."""
from __future__ import annotations

import numpy as np
import torch

from oracle import paramgen as pg
from tests import cap_beam_oracle as cbo
from tests import pos_diverse_oracle as pdo
from tests import util

LP_TOL, LIVE, MARGIN = cbo.LP_TOL, cbo.LIVE, cbo.MARGIN


@torch.no_grad()
def beam_captions_diverse(Pn, xn, L, Gd, Wg, lam, suppress_token=1, dtype=torch.float32, top_n_only=False):
    """The search in `dtype` over the batch xn (one entry per pair).  Returns pos_diverse_oracle.gather_result's dict: seq
    (P,Gd,Wg,L) int64, logp, score (P,Gd,Wg), trace (P,L,N,2) int32 with pair slot parents, and PairSearch's counters.
    top_n_only: every row cut to its N best (everything else at -3000) before the merge -- the kernel's route."""
    N = Gd * Wg
    with cbo._default_dtype(dtype):
        P, x, running = cbo._cast(Pn, xn, dtype)
        rows = cbo._Rows(P, x, running, N)
        ps = None
        for t in range(L):
            lpn = rows.step().numpy().copy()
            if ps is None:
                ps = [pdo.PairSearch(Gd, Wg, L, lpn.dtype, lam) for _ in range(rows.B)]
            if suppress_token >= 0:
                lpn[:, :, suppress_token] -= 1000
            if top_n_only:
                lpn = np.stack([top_n_rows(r, N) for r in lpn])
            par, nxt = zip(*[ps[b].feed(lpn[b]) for b in range(rows.B)])
            rows.select(np.array(par), np.array(nxt))
    return pdo.gather_result(ps, lpn.dtype)


def top_n_rows(lp, N):
    """The rows with everything outside their N best (larger first, lower word first on ties) at -3000."""
    ix = np.argsort(-lp, axis=1, kind="stable")[:, :N]
    out = np.full_like(lp, -3000)
    np.put_along_axis(out, ix, np.take_along_axis(lp, ix, 1), 1)
    return out


def check_admissible(trace, r, score, seq, Pn, xn, L, Gd, Wg, lam, suppress_token=1):
    """trace (P,L,N,2), r = the returned seq_logp (P,Gd,Wg,L), score (P,Gd,Wg), seq (P,Gd,Wg,L) as numpy, over the repeated batch
    xn.  Returns (group steps checked, float64 liveness (P,L,N))."""
    pdo.trace_in_range(trace, C=Pn["logit.bias"].shape[0], L=L, Gd=Gd, Wg=Wg)
    lp_all = cbo.logps_along_trace(Pn, xn, trace, torch.float64)
    return pdo.check_admissible_groups(trace, r, score, seq, lp_all, L=L, Gd=Gd, Wg=Wg, lam=lam, suppress=suppress_token)


# ---- the cases of tests/test_gpu_cap_diverse.py, shared with tests/test_cap_diverse_cpu.py, which pins their preconditions on the
# float64 oracle.  name -> (dims, eos parameters, logit_gain, input seed, S, Gd, Wg); logit_gain None: the default; 128: chosen on
# the CPU, as PINNED in tests/test_gpu_cap_beam_control.py, so that the float64 margin pins at least one pair of the case
CASES = {
    "tiny_s3g2w2": (util.CFG["tiny"], False, None, 1, 3, 2, 2),
    "tiny_s1g3w1": (util.CFG["tiny"], False, None, 2, 1, 3, 1),          # groups of one slot; one template per video
    "eos_s2g3w1": (util.CFG["tiny"], True, None, 2, 2, 3, 1),            # beams finish early: a finished group's dead slot beside live ones
    "eos_s2g2w2": (util.CFG["tiny"], True, None, 2, 2, 2, 2),
    "mid_s2g2w4": (util.CFG["mid"], False, 128.0, 3, 2, 2, 4),            # N = 8: 64 table entries per pair; the packed step
    "mid_s2g4w2": (util.CFG["mid"], False, None, 4, 2, 4, 2),
    "mideos_s2g4w2": (util.CFG["mid"], True, None, 2, 2, 4, 2),
    "odd_s2g2w2": (util.CFG["odd"], False, None, 5, 2, 2, 2),            # A = 37, R = 20: the scalar state gather; V = 37
    "one_s2g2w2": (util.CFG["one"], False, None, 6, 2, 2, 2),            # L = 1, K = 1, V = 5
    "tiny_s2g8w1": (util.CFG["tiny"], False, None, 7, 2, 8, 1),          # eight groups in series
    "v20001_g2w3": (dict(util.CFG["c1"], B=2, V=20001, L=8), False, 128.0, 8, 1, 2, 3),   # the real layer sizes; 80 KB of staged logits
}
LAMBDA = 0.5


def make_pos(d, S, seed):
    """(B,S,R) float32: S different POS vectors per video."""
    return np.stack([pg.make_inputs(d, seed=seed + 101 * (s + 1))["pos_feats"] for s in range(S)], 1)


def repeated(x, pos):
    """The numpy batch in which video b is repeated S times, with pos_feats row b S + s."""
    S = pos.shape[1]
    xr = {k: np.repeat(v, S, 0) for k, v in x.items()}
    xr["pos_feats"] = np.ascontiguousarray(pos.reshape(-1, pos.shape[2]))
    return xr


def case(name):
    """(d, P, x, pos (B,S,R), Gd, Wg) of a case."""
    dd, eos, gain, seed, S, Gd, Wg = CASES[name]
    d = pg.make_dims(**dd)
    P = util.eos_params(d) if eos else (pg.make_params(d) if gain is None else pg.make_params(d, logit_gain=gain))
    return d, P, pg.make_inputs(d, seed=seed, ragged=not eos), make_pos(d, S, seed), Gd, Wg
