"""Diverse POS beam search on the MI355X: PosModel.beam_templates_diverse (include/xgate_pos_beam_diverse.h) judged everywhere -- no
group excused -- by tests/pos_diverse_oracle.check_admissible_groups, a float64 replay (eager torch on the same GPU) of the KERNEL'S
OWN (token, parent) trace that rebuilds the penalties from the trace and asserts every selection of every group was a legal one
within the rounding of the numbers it was made from.  Then the three exact consequences of the rule (one group is the plain search,
trace included; no penalty repeats the plain search in every group; a penalty of 1000 keeps the live tags of a video's groups
apart), the float64 search's own trace where its margin pins it, workspace and trace independence, every ValueError, and the
control wrapper against its parts done by hand.

The cases and their preconditions (pinned on the CPU): tests/pos_diverse_oracle.CASES, tests/test_pos_diverse_cpu.PRE.
Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import pos_beam_oracle as pbo
from tests import pos_diverse_oracle as pdo
from tests import pos_oracle as po
from tests.pos_control_oracle import cuda_inputs, pos_model
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
F64 = torch.float64
LP_TOL = pbo.LP_TOL


def _search(m, x, Gd, Wg, lam, **kw):
    with torch.no_grad():
        out = m.beam_templates_diverse(*cuda_inputs(x), Gd, Wg, diversity=lam, **kw)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in out]


def _f64(P, run, x):
    Pt, rt = po.to_torch(P, F64, "cuda"), po.to_torch(run, F64, "cuda")
    return Pt, rt, [torch.from_numpy(x[k]).to("cuda", F64) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


def _admissible(d, P, run, x, Gd, Wg, lam, tm, lp, score, trace, suppress=1):
    """(group steps checked, float64 liveness (B,L,N)) of the kernel's own search."""
    pdo.trace_in_range(trace, C=d.C, L=d.L, Gd=Gd, Wg=Wg)
    Pt, rt, f = _f64(P, run, x)
    lp_all = pbo.logps_along_trace(Pt, rt, *f, trace)
    return pdo.check_admissible_groups(trace, lp, score, tm, lp_all, L=d.L, Gd=Gd, Wg=Wg, lam=lam, suppress=suppress)


def _shape_checks(d, Gd, Wg, tm, lp, score, mk, trace):
    assert tm.shape == (d.B, Gd, Wg, d.L) and tm.dtype == np.int64 and lp.shape == tm.shape and score.shape == (d.B, Gd, Wg)
    assert mk.shape == (d.B, Gd, Wg, d.L + 1) and trace.shape == (d.B, d.L, Gd * Wg, 2) and trace.dtype == np.int32
    assert tm.min() >= 0 and tm.max() < d.C
    assert np.array_equal(mk, pbo.masks_of(tm).astype(np.float32))
    assert (score[:, :, :-1] >= score[:, :, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()


# ---- 1. the kernel's own search, judged in float64, over every case; the float64 search's trace where its margin pins it
@pytest.mark.parametrize("name", list(pdo.CASES))
def test_own_trace_is_admissible(name):
    from tests.test_pos_diverse_cpu import PRE
    d, P, run, x, Gd, Wg = pdo.case(name)
    lam = pdo.LAMBDA
    tm, lp, score, mk, trace = _search(pos_model(d, P, run), x, Gd, Wg, lam, trim=False, return_trace=True)
    _shape_checks(d, Gd, Wg, tm, lp, score, mk, trace)
    checked, live = _admissible(d, P, run, x, Gd, Wg, lam, tm, lp, score, trace)
    assert checked >= d.B * Gd * 2
    # a beam's score is its penalised sum: at most the sum of its own unpenalised log-probabilities (live beams; the penalty is >= 0)
    ok = score > pbo.LIVE
    assert ok.any() and (score[ok] <= lp.astype(np.float64).sum(3)[ok] + d.L * 1e-5).all()
    Pt, rt, f = _f64(P, run, x)
    o = pdo.beam_templates_diverse(Pt, rt, *f, d.L, Gd, Wg, lam)
    pinned = np.flatnonzero(o["margin"] >= pbo.MARGIN)
    print("%s: %d group steps checked, %d of %d videos pinned" % (name, checked, len(pinned), d.B))
    assert len(pinned) == PRE[name][0][3]                        # a condition of the case, fixed on the CPU
    for b in pinned:
        assert np.array_equal(trace[b], o["trace"][b]) and np.array_equal(tm[b], o["templates"][b]), b
        np.testing.assert_allclose(lp[b], o["tag_logp"][b], atol=LP_TOL)
        np.testing.assert_allclose(score[b], o["score"][b], atol=(d.L + 1) * LP_TOL)


# ---- 2. consequence 1: one group is the plain search, bit for bit, whatever the penalty
@pytest.mark.parametrize("name,W", [("tiny_g2w2", 3), ("tiny_g5w1", 5), ("mid_g2w4", 8), ("eos_g2w2", 3), ("c65", 4), ("c130", 4),
                                    ("c1_g2w3", 5)])
def test_one_group_is_the_plain_search_bit_for_bit(name, W):
    d, P, run, x, _, _ = pdo.case(name)
    m = pos_model(d, P, run)
    with torch.no_grad():
        want = [v.cpu().numpy() for v in m.beam_templates(*cuda_inputs(x), beam_size=W, trim=False, return_trace=True)]
    for lam in (0.0, 0.7, 1000.0):
        got = _search(m, x, 1, W, lam, trim=False, return_trace=True)
        for g, w, what in zip(got, want, ("templates", "tag_logp", "score", "masks", "trace")):
            assert np.array_equal(g.reshape(w.shape), w), (lam, what)


# ---- 3. consequence 2: without a penalty every group is the plain search at W = Wg, bit for bit
@pytest.mark.parametrize("name", ["tiny_g2w2", "tiny_g5w1", "mid_g4w2", "mid_g2w4", "eos_g3w1", "eos_g4w2", "c65", "c1_g2w3"])
def test_without_a_penalty_every_group_is_the_plain_search_bit_for_bit(name):
    """Wg >= 2: exact.  At Wg = 1 the plain search is another instantiation of the step -- with one row per video its attention is
    pos_attn_kernel, the form that makes a one-row call bit-identical to the greedy rollout, where N >= 2 rows per video take
    pos_attn_group_kernel -- and its log-probabilities differ from a group's in the last bit (measured: tiny_g5w1 and eos_g3w1,
    1 ulp in tag_logp).  There the groups are bit-equal to ONE ANOTHER, the search is judged by the float64 admissibility check at
    lambda = 0, and it agrees with the plain search within the log-probability bound on the videos whose float64 margin pins
    them (docs/CAPTION_DIVERSE.md, Checks)."""
    d, P, run, x, Gd, Wg = pdo.case(name)
    m = pos_model(d, P, run)
    with torch.no_grad():
        want = [v.cpu().numpy() for v in m.beam_templates(*cuda_inputs(x), beam_size=Wg, trim=False, return_trace=True)]
    tm, lp, score, mk, trace = _search(m, x, Gd, Wg, 0.0, trim=False, return_trace=True)
    local = [trace[:, :, j * Wg:(j + 1) * Wg] - np.array([0, j * Wg], np.int32) for j in range(Gd)]
    for j in range(Gd):                                          # the groups of a video: one search, Gd times
        for g, what in zip((tm, lp, score, mk), ("templates", "tag_logp", "score", "masks")):
            assert np.array_equal(g[:, j], g[:, 0]), (j, what)
        assert np.array_equal(local[j], local[0]), j
    got = (tm[:, 0], lp[:, 0], score[:, 0], mk[:, 0], local[0])
    if Wg >= 2:
        for g, w, what in zip(got, want, ("templates", "tag_logp", "score", "masks", "trace")):
            assert np.array_equal(g, w), what
        return
    assert _admissible(d, P, run, x, Gd, Wg, 0.0, tm, lp, score, trace)[0] >= d.B * Gd * 2
    Pt, rt, f = _f64(P, run, x)
    pinned = np.flatnonzero(pbo.beam_templates(Pt, rt, *f, d.L, Wg)["margin"] >= pbo.MARGIN)
    assert len(pinned) >= d.B // 2
    assert np.array_equal(got[0][pinned], want[0][pinned]) and np.array_equal(got[4][pinned], want[4][pinned])
    np.testing.assert_allclose(got[1][pinned], want[1][pinned], atol=LP_TOL)
    np.testing.assert_allclose(got[2][pinned], want[2][pinned], atol=(d.L + 1) * LP_TOL)


# ---- 4. consequence 3: a penalty of 1000 keeps the live tags of a video's groups apart at every step
@pytest.mark.parametrize("name", ["tiny_g2w2", "tiny_g5w1", "a_r_odd", "mid_g4w2", "mid_g8w1", "eos_g3w1", "eos_g4w2", "c64", "c130"])
def test_a_large_penalty_keeps_the_live_tags_apart(name):
    d, P, run, x, Gd, Wg = pdo.case(name)
    tm, lp, score, mk, trace = _search(pos_model(d, P, run), x, Gd, Wg, 1000.0, trim=False, return_trace=True)
    _shape_checks(d, Gd, Wg, tm, lp, score, mk, trace)
    checked, live = _admissible(d, P, run, x, Gd, Wg, 1000.0, tm, lp, score, trace)
    assert checked >= d.B * Gd
    assert pdo.live_tokens_disjoint(trace, live, Gd=Gd, Wg=Wg) >= d.B       # (pair, step) with live slots in several groups


# ---- 5. determinism, the workspace, the optional outputs
def test_two_calls_a_poisoned_workspace_and_no_trace_give_the_same_bits():
    d, P, run, x, Gd, Wg = pdo.case("mid_g2w4")
    m = pos_model(d, P, run)
    a, b = (_search(m, x, Gd, Wg, 0.5, trim=False, return_trace=True) for _ in range(2))
    for v, w in zip(a, b):
        assert np.array_equal(v, w)
    small = _search(m, x, 2, 2, 0.5, trim=False, return_trace=True)
    n_big = m._cws.numel()
    m._cws = torch.full((n_big + 4096,), 0xFF, dtype=torch.uint8, device="cuda")       # NaNs and -1s, and larger
    ws = m._cws
    c, small2 = _search(m, x, Gd, Wg, 0.5, trim=False, return_trace=True), _search(m, x, 2, 2, 0.5, trim=False, return_trace=True)
    assert m._cws is ws                                          # the same, larger, poisoned workspace served both calls
    for v, w in zip(a + small, c + small2):
        assert np.array_equal(v, w)
    # without the trace, and trimmed: the same bits
    tm, lp, score, mk = _search(m, x, Gd, Wg, 0.5, trim=False)
    assert np.array_equal(tm, a[0]) and np.array_equal(lp, a[1]) and np.array_equal(score, a[2]) and np.array_equal(mk, a[3])
    n = min(d.L, int((tm != 0).cumprod(3).sum(3).max()))
    tm_t, lp_t, score_t, mk_t = _search(m, x, Gd, Wg, 0.5)
    assert tm_t.shape == (d.B, Gd, Wg, n) and mk_t.shape == (d.B, Gd, Wg, n + 1)
    assert np.array_equal(tm_t, tm[..., :n]) and np.array_equal(lp_t, lp[..., :n]) and np.array_equal(mk_t, mk[..., :n + 1])
    assert (tm[..., n:] == 0).all() and np.array_equal(score_t, score)


def test_bad_arguments_raise():
    d, P, run, x, _, _ = pdo.case("tiny_g2w2")                    # C = 5
    m = pos_model(d, P, run)
    f = cuda_inputs(x)
    for Gd, Wg in ((0, 2), (2, 0), (-1, -1), (2, 3), (3, 2), (6, 1), (1, 6), (9, 1)):
        with pytest.raises(ValueError, match="groups"):
            m.beam_templates_diverse(*f, Gd, Wg)
    for lam in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="diversity"):
            m.beam_templates_diverse(*f, 2, 2, diversity=lam)
    with pytest.raises(ValueError, match="suppress_tag"):
        m.beam_templates_diverse(*f, 2, 2, suppress_tag=5)
    m.train()
    with pytest.raises(NotImplementedError):
        m.beam_templates_diverse(*f, 2, 2)


# ---- 6. into the forced call and the captioner
def test_flattened_templates_feed_the_forced_call_and_caption_beam_diverse_is_its_parts():
    from controllable_xgating_amd import caption_beam_diverse, caption_with_templates, first_occurrences
    dp = po.make_dims(**po.POS_CFG["mid"])
    dc = pg.make_dims(**CFG["mid"])
    assert (dp.K, dp.R, dp.F1, dp.F2) == (dc.K, dc.R, dc.F1, dc.F2)
    Gd, Wg = 2, 2
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    pm = pos_model(dp, P, run)
    Pc = pg.make_params(dc)
    Pc["lstmcore.lstm_1.a2h.weight"] = Pc["lstmcore.lstm_1.a2h.weight"] * np.float32(16.0)      # captions that move with the POS vector
    cap = make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, slp, tm, score, first = caption_beam_diverse(pm, cap, fr, fo, fm, Gd, Wg, diversity=0.5, opt={"sample_max": 1})
    N = Gd * Wg
    assert not any(t.requires_grad for t in (seq, slp, score))
    assert seq.shape[:2] == (dp.B, N) and slp.shape == seq.shape and tm.shape == (dp.B, N, dp.L) and score.shape == (dp.B, N)
    with torch.no_grad():
        tm2, lp2, score2, mk2 = pm.beam_templates_diverse(fr, fo, fm, Gd, Wg, diversity=0.5, trim=False)
        lp_f, _, mk_f, _ = pm.sample_forced(fr, fo, fm, tm2.flatten(1, 2), collect_states=False, trim=False)
    assert torch.equal(tm, tm2.flatten(1, 2)) and torch.equal(score, score2.flatten(1, 2))
    assert torch.equal(first, first_occurrences(tm)) and first[:, 0].all()
    # the forced replay scores the templates as the search did: the unpenalised log-probabilities
    assert torch.equal(mk_f, mk2.flatten(1, 2))
    a, b = lp2.flatten(1, 2).cpu().numpy(), lp_f.cpu().numpy()
    live = a > pbo.LIVE
    np.testing.assert_allclose(b[live], a[live], atol=LP_TOL)
    seq_w, slp_w, _ = caption_with_templates(pm, cap, fr, fo, fm, tm, {"sample_max": 1})
    assert torch.equal(seq, seq_w) and torch.equal(slp, slp_w)
    # the penalty buys distinct templates: more first occurrences than the plain search's four best give at the same width
    with torch.no_grad():
        plain = pm.beam_templates(fr, fo, fm, beam_size=N, trim=False)[0]
    print("distinct templates per video: diverse %s, plain %s" % (first.sum(1).tolist(), first_occurrences(plain).sum(1).tolist()))
