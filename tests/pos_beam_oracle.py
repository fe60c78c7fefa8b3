"""TEST INFRASTRUCTURE ONLY -- POS beam search (include/xgate_pos_beam.h) restated on top of tests/pos_oracle.py: the reference's
sample_beam (pos_src/SAModel.py:104-134, pos_src/CaptionModel.py:22-125) with the done beams ranked by their score at the moment
they finished.  It runs in the dtype and on the device of its inputs (float32 on the CPU against the fixtures
tests/golden/pos_beam_*.npz, float64 in eager torch on a GPU as the high-precision reference of tests/test_gpu_pos_beam.py); the
merge itself (steps 3-5, a few dozen numbers per video) runs in numpy in that dtype, and tools/gen_pos_beam_golden.py replays the
reference's own log-probabilities through it.

`check_admissible` judges a search the KERNEL made, where margins are too tight to pin its tokens: it replays the kernel's own
(token, parent) trace in float64 and asserts that every selection was a legal one within the rounding of the numbers it was made
from."""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import pos_oracle as po

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LP_TOL = 3e-4                                 # the project's log-probability bound
LIVE = -500.0                                 # a candidate below this carries a -1000: a dead slot or the suppressed tag
MARGIN = 1e-3                                 # fixture videos with at least this selection margin have their tokens pinned
# fixture tests/golden/pos_beam_<name>.npz -> (tests/golden/pos_<case>.npz's case, W)
BEAM_CASES = {"tiny_w3": ("tiny", 3), "tiny_w5": ("tiny", 5), "eos_w3": ("eos", 3), "eos_w5": ("eos", 5), "c1_w5": ("c1", 5)}


def merge_step(lp, sums, t, W):
    """Steps 3-4 for one video.  lp (W,C) numpy, the -1000 applied; sums (W).  Returns (q (W,), c (W,), r (W,), p (W,)) of the new
    slots 0 .. W-1, and the sorted p of ALL candidates plus each row's sorted log-probabilities (for margins)."""
    C = lp.shape[1]
    cols, rows = min(W, C), (1 if t == 0 else W)
    ix = np.argsort(-lp[:rows], axis=1, kind="stable")            # descending, lower category first on ties
    ys = np.take_along_axis(lp[:rows], ix, 1)
    cq = np.tile(np.arange(rows), cols)                           # candidate c_rank * rows + q
    cc = np.repeat(np.arange(cols), rows)
    r = ys[cq, cc]
    p = (sums[cq] + r).astype(lp.dtype)                           # one add in the working precision
    order = np.argsort(-p, kind="stable")
    sel = order[:W]
    return cq[sel], ix[cq[sel], cc[sel]], r[sel], p[sel], p[order], ys


def step_margin(p_sorted, ys, W):
    """The smallest gap that decides the step: between adjacent candidates among the first W + 1 after the sort, and between a
    row's `cols`-th and next log-probability."""
    cols = min(W, ys.shape[1])
    head = p_sorted[:W + 1].astype(np.float64)
    m = float(np.min(head[:-1] - head[1:])) if head.size > 1 else np.inf
    if ys.shape[1] > cols:
        m = min(m, float(np.min(ys[:, cols - 1].astype(np.float64) - ys[:, cols].astype(np.float64))))
    return m


class VideoSearch:
    """Steps 3-5 and the result of ONE video, fed one step's (W,C) log-probabilities at a time."""

    def __init__(self, W, L, dtype):
        self.W, self.L, self.t = W, L, 0
        self.sums = np.zeros(W, dtype)
        self.seq = np.zeros((L, W), np.int64)
        self.lps = np.zeros((L, W), dtype)
        self.trace = np.zeros((L, W, 2), np.int32)
        self.done = []                                            # completion order: dict(t, slot, score, seq, logps)
        self.margin = np.inf

    def feed(self, lp):
        """lp (W,C), the -1000 applied.  Returns the parents (W,) and the tokens (W,) of the new slots."""
        W, L, t = self.W, self.L, self.t
        q, c, r, p, p_sorted, ys = merge_step(lp, self.sums, t, W)
        if (p > LIVE).any():
            self.margin = min(self.margin, step_margin(p_sorted, ys, W))
        self.seq[:t] = self.seq[:t, q]
        self.lps[:t] = self.lps[:t, q]
        self.seq[t], self.lps[t] = c, r
        self.trace[t, :, 0], self.trace[t, :, 1] = c, q
        self.sums = p.copy()
        for v in range(W):
            if c[v] == 0 or t == L - 1:
                self.done.append(dict(t=t, slot=v, score=p[v], seq=self.seq[:, v].copy(), logps=self.lps[:, v].copy()))
                self.sums[v] = -1000
        self.t += 1
        return q, c

    def result(self):
        """The done list stable-sorted by score descending, first W."""
        order = np.argsort(-np.array([e["score"] for e in self.done]), kind="stable")[:self.W]
        return [self.done[i] for i in order]


def masks_of(templates):
    """(.., L) tokens -> (.., L+1): column 0 is 1, column t is 1 while the first t tokens are all non-zero."""
    t = np.asarray(templates)
    lead = np.cumprod(t != 0, axis=-1)
    return np.concatenate([np.ones(t.shape[:-1] + (1,), lead.dtype), lead], -1)


@torch.no_grad()
def beam_templates(P, run, fr, fo, fm, L, W, suppress_tag=1):
    """Returns a dict: templates (B,W,L) int64, tag_logp (B,W,L), score (B,W), masks (B,W,L+1), n, trace (B,L,W,2) int32, tokens
    (B,L,W), logps (B,L,W,C) (before the -1000), done (per video, completion order) and margin (B,) -- numpy, in the dtype of the
    inputs."""
    B = fr.shape[0]
    V, q, h, c = po._prologue(P, run, fr, fo, fm)
    V, q, h, c = (x.repeat_interleave(W, 0) for x in (V, q, h, c))
    M = B * W
    one = torch.ones(M, 1, dtype=fr.dtype, device=fr.device)
    tok = torch.zeros(M, dtype=torch.int64, device=fr.device)
    base = (torch.arange(B, device=fr.device) * W).unsqueeze(1)
    vs = None
    logps = []
    for t in range(L):
        h, c, lp = po.step(P, V, q, tok, one, h, c)
        lpn = lp.reshape(B, W, -1).cpu().numpy()
        if vs is None:
            vs = [VideoSearch(W, L, lpn.dtype) for _ in range(B)]
        logps.append(lpn.copy())
        if suppress_tag >= 0:
            lpn[:, :, suppress_tag] -= 1000
        par, nxt = zip(*[vs[b].feed(lpn[b]) for b in range(B)])
        rows = (torch.as_tensor(np.array(par), device=fr.device) + base).reshape(M)
        h, c = h[rows], c[rows]
        tok = torch.as_tensor(np.array(nxt), device=fr.device).reshape(M)
    res = [v.result() for v in vs]
    templates = np.array([[e["seq"] for e in r] for r in res])
    masks = masks_of(templates).astype(logps[0].dtype)
    trace = np.array([v.trace for v in vs])
    return dict(templates=templates, tag_logp=np.array([[e["logps"] for e in r] for r in res]),
                score=np.array([[e["score"] for e in r] for r in res]), masks=masks,
                n=min(L, int((templates != 0).cumprod(2).sum(2).max())), trace=trace, tokens=trace[..., 0].astype(np.int64),
                logps=np.stack(logps, 1), done=[v.done for v in vs], ranked=res, margin=np.array([v.margin for v in vs]))


def backtrace(trace_b, t, slot):
    """The tokens (L,) of the beam that sat in `slot` after step t, and the slot it sat in at every step, from one video's trace
    (L,W,2)."""
    L = trace_b.shape[0]
    seq, slots = np.zeros(L, np.int64), np.zeros(L, np.int64)
    for i in range(t, -1, -1):
        seq[i], slots[i] = trace_b[i, slot, 0], slot
        slot = trace_b[i, slot, 1]
    return seq, slots


@torch.no_grad()
def logps_along_trace(P, run, fr, fo, fm, trace):
    """(B,L,W,C) numpy: the log-probabilities (before the -1000) every step's merge sees when the states are teacher-forced along a
    given search: slot v of step t continues slot trace[b,t,v,1] and is fed the token trace[b,t,v,0]."""
    trace = np.asarray(trace)
    B, L, W, _ = trace.shape
    V, q, h, c = po._prologue(P, run, fr, fo, fm)
    V, q, h, c = (x.repeat_interleave(W, 0) for x in (V, q, h, c))
    M = B * W
    one = torch.ones(M, 1, dtype=fr.dtype, device=fr.device)
    tok = torch.zeros(M, dtype=torch.int64, device=fr.device)
    base = (torch.arange(B, device=fr.device) * W).unsqueeze(1)
    out = []
    for t in range(L):
        h, c, lp = po.step(P, V, q, tok, one, h, c)
        out.append(lp.reshape(B, W, -1))
        rows = (torch.as_tensor(trace[:, t, :, 1].astype(np.int64), device=fr.device) + base).reshape(M)
        h, c = h[rows], c[rows]
        tok = torch.as_tensor(trace[:, t, :, 0].astype(np.int64), device=fr.device).reshape(M)
    return torch.stack(out, 1).cpu().numpy()


def check_admissible(trace, r, score, templates, along, *, C, L, W, suppress_tag):
    """The kernel's own search, judged in float64.  trace (B,L,W,2), r = the returned tag_logp (B,W,L), score (B,W), templates
    (B,W,L) as numpy; along: a callable trace -> the float64 log-probabilities (B,L,W,C), before the -1000, of the states
    teacher-forced along the kernel's parents and tokens (logps_along_trace here, the captioner's in tests/cap_beam_oracle.py),
    called once the trace's indices are known to be in range.  At every step at which a video selects at least one candidate with
    p > -500, for EVERY selected slot: the token is among its parent row's `cols` largest within 3e-4, its float64 p is at least
    the W-th largest float64 p - eps_t, the selected slots descend within eps_t (eps_t = 2 (t + 1) 3e-4: two sums of t + 1
    log-probabilities, each within the bound), and no (parent, token) pair is taken twice.  Then the returned beams: each is a
    distinct completion of the trace with its tokens verbatim, every r within 3e-4 and its score within eps_t of the float64
    one; scores descend, equal scores in completion order, and no completion left out beats a returned one by more than eps.
    Returns the number of (video, step) pairs checked."""
    sup, Cn = suppress_tag, C
    trace, r, score, templates = np.asarray(trace), np.asarray(r), np.asarray(score), np.asarray(templates)
    B = trace.shape[0]
    assert trace.shape == (B, L, W, 2) and r.shape == (B, W, L) and score.shape == (B, W) and templates.shape == (B, W, L)
    cols = min(W, Cn)
    assert trace[..., 0].min() >= 0 and trace[..., 0].max() < Cn and trace[..., 1].min() >= 0 and trace[..., 1].max() < W
    assert (trace[:, 0, :, 1] == 0).all()                         # one row at t = 0
    lp_all = along(trace)
    assert lp_all.dtype == np.float64 and lp_all.shape == (B, L, W, Cn)
    sums = np.zeros((B, W))
    r64 = np.zeros((B, L, W))
    events = [[] for _ in range(B)]                               # completion order: (t, slot, float64 score)
    checked = 0
    for t in range(L):
        lp = lp_all[:, t].copy()
        if sup >= 0:
            lp[:, :, sup] -= 1000
        rows = 1 if t == 0 else W
        eps = 2 * (t + 1) * LP_TOL
        tk, par = trace[:, t, :, 0].astype(np.int64), trace[:, t, :, 1].astype(np.int64)
        ys = -np.sort(-lp[:, :rows], axis=2)[:, :, :cols]                                   # (B,rows,cols)
        cand = (sums[:, :rows, None] + ys).reshape(B, -1)
        wth = -np.sort(-cand, axis=1)[:, W - 1]
        bi = np.arange(B)[:, None]
        rr = lp[bi, par, tk]                                                                # (B,W)
        p = sums[bi, par] + rr
        r64[:, t] = rr
        for b in range(B):
            if not (p[b] > LIVE).any():
                continue
            checked += 1
            where = "video %d step %d" % (b, t)
            assert (rr[b] >= ys[b, par[b], cols - 1] - LP_TOL).all(), (where, "a token outside its row's top", rr[b], ys[b])
            assert (p[b] >= wth[b] - eps).all(), (where, "a selected candidate below the W-th best", p[b], wth[b])
            assert (p[b, :-1] >= p[b, 1:] - eps).all(), (where, "slots out of order", p[b])
            assert len({(int(a), int(k)) for a, k in zip(par[b], tk[b])}) == W, (where, "a candidate taken twice")
        sums = p.copy()
        fin = (tk == 0) | (t == L - 1)
        for b, v in zip(*np.nonzero(fin)):
            events[b].append((t, int(v), p[b, v]))
        sums[fin] = -1000
    for b in range(B):
        ev = events[b]
        assert len(ev) >= W
        beams = [backtrace(trace[b], t, v) for t, v, _ in ev]
        used = []
        for k in range(W):
            # the completion this returned beam is: its tokens verbatim and its score, among those not used yet
            match = [i for i, (t, v, p64) in enumerate(ev) if i not in used and np.array_equal(beams[i][0], templates[b, k]) and
                     abs(p64 - score[b, k]) <= 2 * (t + 1) * LP_TOL]
            assert match, ("video %d rank %d is no completion of the trace" % (b, k), templates[b, k], score[b, k], ev)
            i = match[0]
            used.append(i)
            t, v, p64 = ev[i]
            path = r64[b, np.arange(t + 1), beams[i][1][:t + 1]]
            np.testing.assert_allclose(r[b, k, :t + 1], path, atol=LP_TOL, err_msg="video %d rank %d" % (b, k))
            assert (r[b, k, t + 1:] == 0).all() and (templates[b, k, t + 1:] == 0).all()
        assert (score[b, :-1] >= score[b, 1:]).all(), (b, score[b])
        for k in range(W - 1):
            if score[b, k] == score[b, k + 1]:
                assert used[k] < used[k + 1], (b, k, "equal scores out of completion order")
        worst = min(ev[i][2] for i in used)
        for i, (t, v, p64) in enumerate(ev):
            if i not in used:
                assert p64 <= worst + 2 * L * LP_TOL, ("video %d: completion (%d,%d) left out" % (b, t, v), p64, worst)
    return checked


def load_case(name):
    """(d, P, run, x, W, the fixture) of tests/golden/pos_beam_<name>.npz."""
    case, W = BEAM_CASES[name]
    cfg, kw, eos = po.GOLDEN_CASES[case]
    d = po.make_dims(**po.POS_CFG[cfg])
    g = dict(np.load(os.path.join(GOLD, "pos_beam_%s.npz" % name)))
    return d, po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **kw), W, g
