"""TEST INFRASTRUCTURE ONLY -- diverse beam search (include/xgate_pos_beam_diverse.h; the same group rule serves the captioner's
include/xgate_beam_diverse.h) restated in numpy on top of tests/pos_beam_oracle.py: one `VideoSearch` of width Wg per group, the
groups of a pair fed in series, group j's log-probabilities lowered by lambda times the number of LIVE new slots of groups
0 .. j-1 that took the token at the same step.  It runs in the dtype of its inputs (float32 as the kernel's arithmetic, float64 as
the reference).

`check_admissible_groups` judges a search the KERNEL made: it rebuilds the penalties from the trace's own tokens and float64
liveness and then judges every group exactly as pos_beam_oracle.check_admissible judges a video, at W = Wg, with the same
LP_TOL = 3e-4 and eps_t = 2 (t + 1) 3e-4; the returned tag_logp is judged against the UNPENALISED float64 values."""
from __future__ import annotations

import numpy as np
import torch

from tests import pos_beam_oracle as pbo
from tests import pos_oracle as po

LP_TOL, LIVE = pbo.LP_TOL, pbo.LIVE


def penalty_counts(tokens, C):
    """(C,) int: how often each token occurs in `tokens` (the earlier groups' live new slots)."""
    return np.bincount(np.asarray(tokens, np.int64), minlength=C)[:C] if len(tokens) else np.zeros(C, np.int64)


def penalised(lp, n, lam):
    """a = lp - lambda * n in the dtype of lp: one multiply and one subtraction, each rounded on its own."""
    dt = lp.dtype.type
    return (lp - (n.astype(lp.dtype) * dt(lam)).astype(lp.dtype)).astype(lp.dtype)


class PairSearch:
    """One pair's Gd groups, fed one step's (N,C) log-probabilities (the -1000 applied) at a time.  Counters for the tests'
    preconditions: `changed` (group steps whose selection differs from the unpenalised one), `dead_reused` (a dead new slot of an
    earlier group holds a token that a later group's live new slot takes at the same step), `near_dead` (the smallest distance of a
    new sum from -500)."""

    def __init__(self, Gd, Wg, L, dtype, lam):
        self.Gd, self.Wg, self.L, self.lam, self.t = Gd, Wg, L, lam, 0
        self.vs = [pbo.VideoSearch(Wg, L, dtype) for _ in range(Gd)]
        self.trace = np.zeros((L, Gd * Wg, 2), np.int32)
        self.changed = self.dead_reused = 0
        self.near_dead = np.inf
        self.disjoint = True                                      # live slots of different groups never share a token at a step

    def feed(self, lp):
        Gd, Wg, t = self.Gd, self.Wg, self.t
        C = lp.shape[1]
        live_tok, dead_tok = [], []
        par, tok = np.zeros(Gd * Wg, np.int64), np.zeros(Gd * Wg, np.int64)
        for j, vs in enumerate(self.vs):
            rows = lp[j * Wg:(j + 1) * Wg]
            a = penalised(rows, penalty_counts(live_tok, C)[None, :], self.lam)
            plain = pbo.merge_step(rows, vs.sums, t, Wg)
            old = vs.sums.copy()
            n_done = len(vs.done)
            q, c = vs.feed(a)
            if not (np.array_equal(plain[0], q) and np.array_equal(plain[1], c)):
                self.changed += 1
            r = rows[q, c]                                        # the unpenalised log-probability is what is stored
            vs.lps[t] = r
            for e in vs.done[n_done:]:
                e["logps"][t] = r[e["slot"]]
            p = (old[q] + a[q, c]).astype(lp.dtype)
            self.near_dead = min(self.near_dead, float(np.min(np.abs(p.astype(np.float64) - LIVE))))
            mine = [int(v) for v, pv in zip(c, p) if pv > LIVE]
            self.dead_reused += len(set(mine) & set(dead_tok))
            if set(mine) & set(live_tok):
                self.disjoint = False
            live_tok += mine
            dead_tok += [int(v) for v, pv in zip(c, p) if not pv > LIVE]
            par[j * Wg:(j + 1) * Wg], tok[j * Wg:(j + 1) * Wg] = q + j * Wg, c
        self.trace[t, :, 0], self.trace[t, :, 1] = tok, par
        self.t += 1
        return par, tok

    def result(self):
        return [vs.result() for vs in self.vs]


def gather_result(pairs, dtype):
    """The outputs of a list of finished PairSearch as arrays with leading dims (pairs, Gd, Wg)."""
    res = [p.result() for p in pairs]
    seq = np.array([[[e["seq"] for e in g] for g in r] for r in res])
    return dict(seq=seq, logp=np.array([[[e["logps"] for e in g] for g in r] for r in res]).astype(dtype),
                score=np.array([[[e["score"] for e in g] for g in r] for r in res]).astype(dtype),
                trace=np.array([p.trace for p in pairs]), ranked=res,
                finish=[[sorted({e["t"] for e in g}) for g in r] for r in res],
                changed=sum(p.changed for p in pairs), dead_reused=sum(p.dead_reused for p in pairs),
                near_dead=min(p.near_dead for p in pairs), disjoint=all(p.disjoint for p in pairs),
                margin=np.array([min(v.margin for v in p.vs) for p in pairs]))


@torch.no_grad()
def beam_templates_diverse(P, run, fr, fo, fm, L, Gd, Wg, lam, suppress_tag=1):
    """The diverse search over the POS generator in the dtype of the inputs.  Returns a dict: templates (B,Gd,Wg,L) int64, tag_logp,
    score (B,Gd,Wg), masks (B,Gd,Wg,L+1), trace (B,L,N,2) int32 (pair slot parents) and the counters of PairSearch."""
    B, N = fr.shape[0], Gd * Wg
    V, q, h, c = po._prologue(P, run, fr, fo, fm)
    V, q, h, c = (x.repeat_interleave(N, 0) for x in (V, q, h, c))
    M = B * N
    one = torch.ones(M, 1, dtype=fr.dtype, device=fr.device)
    tok = torch.zeros(M, dtype=torch.int64, device=fr.device)
    base = (torch.arange(B, device=fr.device) * N).unsqueeze(1)
    ps = None
    for t in range(L):
        h, c, lp = po.step(P, V, q, tok, one, h, c)
        lpn = lp.reshape(B, N, -1).cpu().numpy()
        if ps is None:
            ps = [PairSearch(Gd, Wg, L, lpn.dtype, lam) for _ in range(B)]
        if suppress_tag >= 0:
            lpn[:, :, suppress_tag] -= 1000
        par, nxt = zip(*[ps[b].feed(lpn[b]) for b in range(B)])
        rows = (torch.as_tensor(np.array(par), device=fr.device) + base).reshape(M)
        h, c = h[rows], c[rows]
        tok = torch.as_tensor(np.array(nxt), device=fr.device).reshape(M)
    o = gather_result(ps, lpn.dtype)
    o["templates"], o["tag_logp"] = o.pop("seq"), o.pop("logp")
    o["masks"] = pbo.masks_of(o["templates"]).astype(lpn.dtype)
    return o


def check_admissible_groups(trace, r, score, seqs, lp_all, *, L, Gd, Wg, lam, suppress):
    """The kernel's own diverse search, judged in float64.  trace (P,L,N,2) with pair slot parents, r = the returned
    log-probabilities (P,Gd,Wg,L), score (P,Gd,Wg), seqs (P,Gd,Wg,L) as numpy; lp_all (P,L,N,C) float64: the log-probabilities,
    before the -1000, of the states teacher-forced along the trace (call `trace_in_range` first).  Per step the groups in order:
    n_j from the trace's own tokens and the float64 liveness of the earlier groups' new slots, a = lp - lambda n_j, and then for
    every group at which at least one selected candidate has p > -500 the assertions of pos_beam_oracle.check_admissible at
    W = Wg; then the returned beams of every group, their r against the UNPENALISED float64 values.  Returns (the number of (pair,
    step, group) triples checked, live (P,L,N) bool: the float64 liveness of every new slot)."""
    trace, r, score, seqs = np.asarray(trace), np.asarray(r), np.asarray(score), np.asarray(seqs)
    Pn, N = trace.shape[0], Gd * Wg
    Cn = lp_all.shape[3]
    assert lp_all.dtype == np.float64 and lp_all.shape == (Pn, L, N, Cn)
    assert r.shape == (Pn, Gd, Wg, L) and score.shape == (Pn, Gd, Wg) and seqs.shape == (Pn, Gd, Wg, L)
    cols = min(Wg, Cn)
    sums = np.zeros((Pn, N))
    r64 = np.zeros((Pn, L, N))
    live = np.zeros((Pn, L, N), bool)
    events = [[[] for _ in range(Gd)] for _ in range(Pn)]        # completion order: (t, local slot, float64 score)
    checked = 0
    for t in range(L):
        eps = 2 * (t + 1) * LP_TOL
        new_sums = sums.copy()
        for b in range(Pn):
            lp = lp_all[b, t].copy()
            if suppress >= 0:
                lp[:, suppress] -= 1000
            live_tok = []
            for j in range(Gd):
                sl = slice(j * Wg, (j + 1) * Wg)
                rows = 1 if t == 0 else Wg
                lpj = lp[j * Wg:j * Wg + rows]
                a = lpj - lam * penalty_counts(live_tok, Cn)[None, :]
                tk, par = trace[b, t, sl, 0].astype(np.int64), trace[b, t, sl, 1].astype(np.int64) - j * Wg
                ys = -np.sort(-a, axis=1)[:, :cols]
                cand = (sums[b, sl][:rows, None] + ys).reshape(-1)
                wth = -np.sort(-cand)[Wg - 1]
                rr = a[par, tk]
                p = sums[b, sl][par] + rr
                r64[b, t, sl] = lpj[par, tk]
                live[b, t, sl] = p > LIVE
                if (p > LIVE).any():
                    checked += 1
                    where = "pair %d step %d group %d" % (b, t, j)
                    assert (rr >= ys[par, cols - 1] - LP_TOL).all(), (where, "a token outside its row's top", rr, ys)
                    assert (p >= wth - eps).all(), (where, "a selected candidate below the Wg-th best", p, wth)
                    assert (p[:-1] >= p[1:] - eps).all(), (where, "slots out of order", p)
                    assert len({(int(x), int(k)) for x, k in zip(par, tk)}) == Wg, (where, "a candidate taken twice")
                live_tok += [int(v) for v, pv in zip(tk, p) if pv > LIVE]
                fin = (tk == 0) | (t == L - 1)
                for v in np.flatnonzero(fin):
                    events[b][j].append((t, int(v), p[v]))
                new_sums[b, sl] = np.where(fin, -1000.0, p)
        sums = new_sums
    for b in range(Pn):
        for j in range(Gd):
            ev = events[b][j]
            assert len(ev) >= Wg
            tr = trace[b, :, j * Wg:(j + 1) * Wg].copy()
            tr[..., 1] -= j * Wg
            beams = [pbo.backtrace(tr, t, v) for t, v, _ in ev]
            used = []
            for k in range(Wg):
                match = [i for i, (t, v, p64) in enumerate(ev) if i not in used and np.array_equal(beams[i][0], seqs[b, j, k]) and
                         abs(p64 - score[b, j, k]) <= 2 * (t + 1) * LP_TOL]
                assert match, ("pair %d group %d rank %d is no completion of the trace" % (b, j, k), seqs[b, j, k], score[b, j, k], ev)
                i = match[0]
                used.append(i)
                t, v, p64 = ev[i]
                path = r64[b, np.arange(t + 1), j * Wg + beams[i][1][:t + 1]]
                np.testing.assert_allclose(r[b, j, k, :t + 1], path, atol=LP_TOL, err_msg="pair %d group %d rank %d" % (b, j, k))
                assert (r[b, j, k, t + 1:] == 0).all() and (seqs[b, j, k, t + 1:] == 0).all()
            sc = score[b, j]
            assert (sc[:-1] >= sc[1:]).all(), (b, j, sc)
            for k in range(Wg - 1):
                if sc[k] == sc[k + 1]:
                    assert used[k] < used[k + 1], (b, j, k, "equal scores out of completion order")
            worst = min(ev[i][2] for i in used)
            for i, (t, v, p64) in enumerate(ev):
                if i not in used:
                    assert p64 <= worst + 2 * L * LP_TOL, ("pair %d group %d: completion (%d,%d) left out" % (b, j, t, v), p64, worst)
    return checked, live


def trace_in_range(trace, *, C, L, Gd, Wg):
    """The trace's indices: tokens in [0, C), the parent of a slot of group j in [j Wg, (j + 1) Wg), j Wg at t = 0."""
    trace = np.asarray(trace)
    N = Gd * Wg
    assert trace.shape[1:] == (L, N, 2) and trace.dtype == np.int32
    assert trace[..., 0].min() >= 0 and trace[..., 0].max() < C
    group0 = (np.arange(N) // Wg) * Wg
    assert (trace[..., 1] >= group0).all() and (trace[..., 1] < group0 + Wg).all()
    assert (trace[:, 0, :, 1] == group0).all()


def live_tokens_disjoint(trace, live, *, Gd, Wg):
    """Consequence 3: at every step the token sets of the live slots of different groups of a pair are disjoint.  trace (P,L,N,2);
    live (P,L,N) bool: whether the slot's new sum at that step is above -500.  Returns the number of (pair, step) with live slots
    in at least two groups."""
    trace, live = np.asarray(trace), np.asarray(live)
    several = 0
    for b in range(trace.shape[0]):
        for t in range(trace.shape[1]):
            sets = [{int(v) for v, lv in zip(trace[b, t, j * Wg:(j + 1) * Wg, 0], live[b, t, j * Wg:(j + 1) * Wg]) if lv}
                    for j in range(Gd)]
            several += sum(1 for s in sets if s) >= 2
            for i in range(Gd):
                for j in range(i + 1, Gd):
                    assert not (sets[i] & sets[j]), ("pair %d step %d: groups %d and %d share a live token" % (b, t, i, j), sets)
    return several


# ---- the cases of tests/test_gpu_pos_diverse.py, shared with tests/test_pos_diverse_cpu.py, which pins their preconditions on the
# float64 oracle.  name -> (dims, eos parameters, input seed, Gd, Wg[, logit_gain]): the shapes of tests/test_gpu_pos_beam.py that reach each
# branch of pos_beam_merge_diverse_kernel and of the launches around it
_SMALL = dict(E=18, C=5, L=6, F1=20, F2=12)
_HEAD = dict(B=2, K=5, R=40, A=52, E=24, L=6, F1=20, F2=12)
CASES = {
    "tiny_g2w2": (po.POS_CFG["tiny"], False, 5, 2, 2),
    "tiny_g3w1": (po.POS_CFG["tiny"], False, 6, 3, 1),                 # groups of one slot: one candidate per group
    "tiny_g5w1": (po.POS_CFG["tiny"], False, 7, 5, 1),                 # N = C: the suppressed tag is a candidate
    "a_r_odd": (dict(B=3, K=5, R=22, A=38, **_SMALL), False, 8, 2, 2),  # A % 4 != 0 (scalar loads), R % 4 != 0
    "mid_g2w4": (po.POS_CFG["mid"], False, 9, 2, 4, 128.0),                   # N = 8: a full attention group and a partial one
    "mid_g4w2": (po.POS_CFG["mid"], False, 10, 4, 2, 128.0),
    "mid_g8w1": (po.POS_CFG["mid"], False, 11, 8, 1),
    "eos_g2w2": (po.POS_CFG["mid"], True, po.EOS_CASE["input_seed"], 2, 2),   # beams finish early: dead slots beside live ones
    "eos_g3w1": (po.POS_CFG["mid"], True, po.EOS_CASE["input_seed"], 3, 1),   # a finished group's dead slot holds a tag a later group takes
    "eos_g4w2": (po.POS_CFG["mid"], True, po.EOS_CASE["input_seed"], 4, 2),
    "c64": (dict(_HEAD, C=64), False, 12, 2, 2, 128.0),                       # the last size of the lane-per-category log-sum-exp
    "c65": (dict(_HEAD, C=65), False, 13, 2, 2),                       # the first size of the serial one; two entries per lane
    "c130": (dict(_HEAD, C=130), False, 14, 3, 2, 128.0),                     # three entries per lane in the re-rank
    "c1_g2w3": (po.POS_CFG["c1"], False, 15, 2, 3, 128.0),                    # the real layer sizes
}
LAMBDA = 0.5


def case(name):
    """(d, P, run, x, Gd, Wg) of a case."""
    dd, eos, seed, Gd, Wg = CASES[name][:5]
    gain = dict(logit_gain=CASES[name][5]) if len(CASES[name]) > 5 else {}      # chosen on the CPU so that a float64 margin pins a video
    d = po.make_dims(**dd)
    return d, po.make_params(d, eos=eos, **gain), po.make_running(d), po.make_inputs(d, seed=seed, ragged=not eos), Gd, Wg
