"""The captioner's diverse beam search on the MI355X: SAModel.beam_captions_diverse (include/xgate_beam_diverse.h) judged on every
case -- no group excused -- by tests/cap_diverse_oracle.check_admissible, a float64 replay of the KERNEL'S OWN (token, parent)
trace on the repeated batch that rebuilds the penalties from the trace and asserts every selection of every group was a legal one
within the rounding of the numbers it was made from.  Then the three exact consequences of the rule (one group is
beam_captions_per_video, trace included; no penalty repeats it in every group; a penalty of 1000 keeps the live words of a pair's
groups apart), the float64 search's own trace where its margin pins the pair, workspace and trace independence, and
control.diverse_beam_captions_with_templates against its parts done by hand.

The cases and their preconditions (pinned on the CPU): tests/cap_diverse_oracle.CASES, tests/test_cap_diverse_cpu.PRE.
Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4."""
import numpy as np
import pytest
import torch

from tests import cap_beam_oracle as cbo
from tests import cap_diverse_oracle as cdo
from tests.util import make_model

pytestmark = pytest.mark.gpu
LP_TOL = cbo.LP_TOL


def _videos(x):
    return tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))


def _search(m, x, pos, Gd, Wg, lam, **kw):
    """beam_captions_diverse, as numpy viewed over the B S pairs: [seq (P,Gd,Wg,L), seq_logp, score (P,Gd,Wg)[, trace (P,L,N,2)]]."""
    B, S = pos.shape[:2]
    with torch.no_grad():
        out = m.beam_captions_diverse(*_videos(x), torch.from_numpy(pos).cuda(), Gd, Wg, diversity=lam, **kw)
    torch.cuda.synchronize()
    assert out[0].shape[:4] == (B, S, Gd, Wg) and out[2].shape == (B, S, Gd, Wg)
    return [v.cpu().numpy().reshape((B * S,) + tuple(v.shape[2:])) for v in out]


def _plain(m, x, pos, W):
    """beam_captions_per_video over the pairs: [seq (P,W,L), seq_logp, score (P,W), trace (P,L,W,2)]."""
    B, S = pos.shape[:2]
    with torch.no_grad():
        out = m.beam_captions_per_video(*_videos(x), torch.from_numpy(pos).cuda(), beam_size=W, return_trace=True)
    torch.cuda.synchronize()
    return [v.cpu().numpy().reshape((B * S,) + tuple(v.shape[2:])) for v in out]


def _shape_checks(Pn, d, Gd, Wg, seq, lp, score, trace):
    assert seq.shape == (Pn, Gd, Wg, d.L) and seq.dtype == np.int64 and lp.shape == seq.shape and score.shape == (Pn, Gd, Wg)
    assert trace.shape == (Pn, d.L, Gd * Wg, 2) and trace.dtype == np.int32
    assert seq.min() >= 0 and seq.max() < d.V
    assert (score[:, :, :-1] >= score[:, :, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()


# ---- 1. the kernel's own search, judged in float64, over every case; the float64 search's trace where its margin pins the pair
@pytest.mark.parametrize("name", list(cdo.CASES))
def test_own_trace_is_admissible(name):
    from tests.test_cap_diverse_cpu import PRE
    d, P, x, pos, Gd, Wg = cdo.case(name)
    lam, xr, Pn = cdo.LAMBDA, cdo.repeated(x, pos), d.B * pos.shape[1]
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, Gd, Wg, lam, return_trace=True)
    _shape_checks(Pn, d, Gd, Wg, seq, lp, score, trace)
    checked, live = cdo.check_admissible(trace, lp, score, seq, P, xr, d.L, Gd, Wg, lam)
    assert checked >= Pn * Gd * min(d.L, 2)
    ok = score > cbo.LIVE                                        # the penalty is >= 0: a score is at most its beam's pure sum
    assert ok.any() and (score[ok] <= lp.astype(np.float64).sum(3)[ok] + d.L * 1e-5).all()
    print("%s: %d group steps checked, %d of %d pairs pinned" % (name, checked, PRE[name][0][3], Pn))
    torch.set_num_threads(8)
    o = cdo.beam_captions_diverse(P, xr, d.L, Gd, Wg, lam, dtype=torch.float64)
    pinned = np.flatnonzero(o["margin"] >= cbo.MARGIN)
    assert len(pinned) == PRE[name][0][3]                        # a condition of the case, fixed on the CPU
    for b in pinned:
        assert np.array_equal(trace[b], o["trace"][b]) and np.array_equal(seq[b], o["seq"][b]), b
        np.testing.assert_allclose(lp[b], o["logp"][b], atol=LP_TOL)
        np.testing.assert_allclose(score[b], o["score"][b], atol=(d.L + 1) * LP_TOL)


# At the real layer sizes the plain search's log-probabilities are not bit-reproducible from call to call: on the same inputs
# repeat calls of beam_captions_per_video (the v20001 case) differed from the first in seq_logp, by up to 1.9e-6, with seq, score
# and trace equal (measured; docs/CAPTION_DIVERSE.md, Checks: the step's fp32 products there take routes that sum partial tiles
# with float atomics).  So at that one case seq and trace are compared exactly and seq_logp and score within the log-probability
# bound, on ALL pairs, and consequence 2 is also judged by the float64 admissibility check at lambda = 0; every other case is
# exact throughout.
NOT_REPRODUCIBLE = {"v20001_g2w3"}


def _assert_same_search(name, got, want, L, where):
    exact = ("seq", "trace") if name in NOT_REPRODUCIBLE else ("seq", "seq_logp", "score", "trace")
    for g, w, what in zip(got, want, ("seq", "seq_logp", "score", "trace")):
        if what in exact:
            assert np.array_equal(g, w), (where, what)
        else:
            np.testing.assert_allclose(g, w, atol=LP_TOL if what == "seq_logp" else (L + 1) * LP_TOL, err_msg=str((where, what)))


# ---- 2. consequence 1: one group is the rows-per-video search, bit for bit, whatever the penalty
@pytest.mark.parametrize("name,W", [("tiny_s3g2w2", 3), ("tiny_s1g3w1", 1), ("eos_s2g2w2", 5), ("mid_s2g2w4", 8), ("odd_s2g2w2", 3),
                                    ("one_s2g2w2", 2), ("v20001_g2w3", 3)])
def test_one_group_is_the_plain_search_bit_for_bit(name, W):
    d, P, x, pos, _, _ = cdo.case(name)
    m = make_model(d, P, train=False)
    want = _plain(m, x, pos, W)
    for lam in (0.0, 0.7, 1000.0):
        got = _search(m, x, pos, 1, W, lam, return_trace=True)
        _assert_same_search(name, [g.reshape(w.shape) for g, w in zip(got, want)], want, d.L, lam)


# ---- 3. consequence 2: without a penalty every group is the rows-per-video search at W = Wg, bit for bit
@pytest.mark.parametrize("name", ["tiny_s3g2w2", "tiny_s1g3w1", "eos_s2g3w1", "eos_s2g2w2", "mid_s2g4w2", "mid_s2g2w4", "odd_s2g2w2",
                                  "one_s2g2w2", "v20001_g2w3"])
def test_without_a_penalty_every_group_is_the_plain_search_bit_for_bit(name):
    d, P, x, pos, Gd, Wg = cdo.case(name)
    m = make_model(d, P, train=False)
    want = _plain(m, x, pos, Wg)
    seq, lp, score, trace = _search(m, x, pos, Gd, Wg, 0.0, return_trace=True)
    for j in range(Gd):
        local = trace[:, :, j * Wg:(j + 1) * Wg] - np.array([0, j * Wg], np.int32)
        _assert_same_search(name, (seq[:, j], lp[:, j], score[:, j], local), want, d.L, j)
        if name not in NOT_REPRODUCIBLE:                         # within one call the groups of a pair are bit-equal to one another
            for g in (seq, lp, score):
                assert np.array_equal(g[:, j], g[:, 0]), j
    if name in NOT_REPRODUCIBLE:
        checked, _ = cdo.check_admissible(trace, lp, score, seq, P, cdo.repeated(x, pos), d.L, Gd, Wg, 0.0)
        assert checked >= len(seq) * Gd * 2


# ---- 4. consequence 3: a penalty of 1000 keeps the live words of a pair's groups apart at every step
@pytest.mark.parametrize("name", ["tiny_s3g2w2", "eos_s2g3w1", "mideos_s2g4w2", "odd_s2g2w2", "one_s2g2w2", "tiny_s2g8w1", "v20001_g2w3"])
def test_a_large_penalty_keeps_the_live_words_apart(name):
    d, P, x, pos, Gd, Wg = cdo.case(name)
    Pn = d.B * pos.shape[1]
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, Gd, Wg, 1000.0, return_trace=True)
    _shape_checks(Pn, d, Gd, Wg, seq, lp, score, trace)
    checked, live = cdo.check_admissible(trace, lp, score, seq, P, cdo.repeated(x, pos), d.L, Gd, Wg, 1000.0)
    assert checked >= Pn * Gd
    assert cdo.pdo.live_tokens_disjoint(trace, live, Gd=Gd, Wg=Wg) >= Pn      # (pair, step) with live slots in several groups
    assert (live[:, 0].reshape(Pn, Gd, Wg)[:, :, 0]).all()                    # every group opens with a live word of its own
    first = trace[:, 0, ::Wg, 0]
    assert all(len(set(r.tolist())) == Gd for r in first)


# ---- 5. the workspace and the trace
def test_result_does_not_depend_on_the_workspace_or_the_trace():
    d, P, x, pos, Gd, Wg = cdo.case("tiny_s3g2w2")
    m = make_model(d, P, train=False)
    first = _search(m, x, pos, Gd, Wg, 0.5, return_trace=True)
    again = _search(m, x, pos, Gd, Wg, 0.5, return_trace=True)
    (key, ws), = m._beam_diverse_ws.items()
    m._beam_diverse_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}   # NaNs and -1s, and larger
    dirty = _search(m, x, pos, Gd, Wg, 0.5, return_trace=True)
    plain = _search(m, x, pos, Gd, Wg, 0.5)
    for a, b_, c in zip(first, again, dirty):
        assert np.array_equal(a, b_) and np.array_equal(a, c)
    assert len(plain) == 3 and all(np.array_equal(a, b_) for a, b_ in zip(first, plain))


# ---- 6. through the control chain
def test_diverse_beam_captions_with_templates_is_the_chain_done_by_hand():
    from controllable_xgating_amd import diverse_beam_captions_with_templates
    from tests.pos_control_oracle import cuda_inputs, pos_model
    from tests.test_gpu_cap_beam_control import CHAIN, chain_case
    dp, dc, P, run, x, tm, Pc, _ = chain_case()
    S, Gd, Wg = CHAIN["S"], 2, 2
    pm, cap = pos_model(dp, P, run), make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, lp, score, tscore = diverse_beam_captions_with_templates(pm, cap, fr, fo, fm, tm, Gd, Wg, diversity=0.5)
    assert seq.shape == (dp.B, S, Gd, Wg, dc.L) and lp.shape == seq.shape and score.shape == (dp.B, S, Gd, Wg) and tscore.shape == (dp.B, S)
    assert not any(t.requires_grad for t in (seq, lp, score, tscore))
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
        want = cap.beam_captions_diverse(fr, fo, fm, pos_feats.reshape(dp.B, S, -1), Gd, Wg, diversity=0.5)
    assert torch.equal(tscore, tag_logp.sum(2))
    for g, w in zip((seq, lp, score), want):
        assert torch.equal(g, w)
