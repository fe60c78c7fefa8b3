"""The captioner's beam search on the MI355X: SAModel.beam_captions (include/xgate_beam.h) against the reference's fixtures
tests/golden/cap_beam_*.npz where their selection margins pin the tokens, and everywhere -- no row excused -- by
tests/cap_beam_oracle.check_admissible: a float64 replay of the KERNEL'S OWN (token, parent) trace that asserts every selection was
a legal one within the rounding of the numbers it was made from.  Then the greedy rollout at W = 1, the host search of beam.py on
the same model, the tie rule and the suppression exactly, workspace independence, and control.caption_beam.

Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_beam_oracle as cbo
from tests.util import CFG, eos_params, load_golden, make_model, to_dev

pytestmark = pytest.mark.gpu
LP_TOL = cbo.LP_TOL

# name -> (dims, W): the smallest shapes that reach each branch of the two new kernels and of the launches around them
CASES = {
    "tiny_w1": (CFG["tiny"], 1),                                # one candidate row, one candidate
    "tiny_w3": (CFG["tiny"], 3),                                # V = 61 < the workgroup, V % 4 != 0; E = 18: the skinny step without packed weights
    "tiny_w5": (CFG["tiny"], 5),
    "tiny_w8": (CFG["tiny"], 8),                                # a full wave of 64 candidates
    "odd_w3": (CFG["odd"], 3),                                  # R = 20: the unpacked step (token rows gathered by a launch); V = 37
    "one_w2": (CFG["one"], 2),                                  # L = 1, K = 1, V = 5: everything finishes at t = 0 with one row
    "mid_w5": (CFG["mid"], 5),                                  # the packed step (tokens by index); V = 500: two workgroup strides
    "mid_w8": (CFG["mid"], 8),
    "mid_rows_150": (dict(CFG["mid"], B=30), 5),                # past 128 rows
    "v4100": (dict(CFG["tiny"], B=2, V=4100), 3),               # one float4 a thread and a second for four threads; 16-byte aligned rows
    "v20001": (dict(CFG["tiny"], B=2, V=20001), 3),             # 80 KB of LDS: the opt-in; V % 4 = 1: every row alignment
    "v38500": (dict(CFG["tiny"], B=2, V=38500), 3),             # past 150 KiB of LDS: the row read three times from memory
    "w_equals_v": (dict(CFG["tiny"], B=3, V=8), 8),             # W = V: the suppressed word and every other is a candidate
    "c1_w5": (dict(CFG["c1"], B=3), 5),                         # the real layer sizes
    "c5_w3": (dict(CFG["c5"], B=2), 3),                         # R = 1024, K = 40
}


def test_cases_reach_the_branches_they_name():
    for name, (d, W) in CASES.items():
        assert 1 <= W <= min(8, d["V"]), name
    assert CASES["odd_w3"][0]["R"] % 8 and not CASES["tiny_w3"][0]["R"] % 8 and CASES["tiny_w3"][0]["E"] % 4
    assert all(CASES["mid_w5"][0][k] % m == 0 for k, m in (("R", 8), ("E", 4), ("A", 4)))
    assert CASES["tiny_w8"][1] ** 2 == 64 and CASES["w_equals_v"][1] == CASES["w_equals_v"][0]["V"]
    assert CASES["mid_rows_150"][0]["B"] * CASES["mid_rows_150"][1] == 150 > 128
    assert CASES["tiny_w3"][0]["V"] < 256 and CASES["tiny_w3"][0]["V"] % 4 and CASES["mid_w5"][0]["V"] > 256
    assert 64 * 1024 < 4 * (CASES["v20001"][0]["V"] + 8) <= 150 * 1024 and CASES["v20001"][0]["V"] % 4 == 1
    assert 4 * (CASES["v4100"][0]["V"] + 8) <= 64 * 1024 and CASES["v4100"][0]["V"] % 4 == 0 and CASES["v4100"][0]["V"] > 4 * 1024
    assert 4 * (CASES["v38500"][0]["V"] + 8) > 150 * 1024
    assert CASES["one_w2"][0]["L"] == 1


def _inputs(x):
    xd = to_dev(x)
    return xd["feats_rgb"], xd["feats_opfl"], xd["feat_mask"], xd["pos_feats"]


def _beam(m, x, W, **kw):
    with torch.no_grad():
        out = m.beam_captions(*_inputs(x), beam_size=W, **kw)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in out]


def _shape_checks(d, W, seq, lp, score, trace):
    assert seq.shape == (d.B, W, d.L) and seq.dtype == np.int64 and lp.shape == seq.shape and score.shape == (d.B, W)
    assert trace.shape == (d.B, d.L, W, 2) and trace.dtype == np.int32
    assert seq.min() >= 0 and seq.max() < d.V
    assert (score[:, :-1] >= score[:, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()


# ---- 1. against the reference's fixtures
@pytest.mark.parametrize("name", list(cbo.BEAM_CASES))
def test_against_the_reference_fixtures(name):
    d, P, x, W, g = cbo.load_case(name)
    seq, lp, score, trace = _beam(make_model(d, P, train=False), x, W, return_trace=True)
    _shape_checks(d, W, seq, lp, score, trace)
    ok = np.flatnonzero(g["margin"] >= cbo.MARGIN)
    print("%s: margins %s -> %d of %d videos pinned" % (name, " ".join("%.1e" % v for v in g["margin"]), len(ok), d.B))
    if name in ("tiny_w3", "eos_w3"):
        assert len(ok) == 4                                      # conditions of the fixtures, not measurements
    replay = cbo.replay_fixture(g, W, d.L)                       # steps 3-5 over the reference's own log-probabilities
    for b in ok:
        assert np.array_equal(trace[b, :, :, 0], g["tokens"][b]), (b, trace[b, :, :, 0], g["tokens"][b])
        assert np.array_equal(trace[b], replay[b].trace), b
        ranked = replay[b].result()
        assert np.array_equal(seq[b], np.array([e["seq"] for e in ranked])), b
        np.testing.assert_allclose(lp[b], np.array([e["logps"] for e in ranked]), atol=LP_TOL)
        for k, e in enumerate(ranked):
            assert abs(score[b, k] - e["score"]) <= (e["t"] + 1) * LP_TOL, (b, k)
    # every video, whatever its margin
    assert cbo.check_admissible(trace, lp, score, seq, P, x, d.L, W) >= d.B


@pytest.mark.parametrize("tag", ["tiny", "c1"])
def test_best_beam_is_the_host_search_fixture(tag):
    """The assertion of the host path's own test (tests/test_gpu_parity.py: test_beam_search_vs_reference_golden)."""
    g = load_golden("beam_%s.npz" % tag)
    d = pg.make_dims(**dict(CFG[tag], B=min(CFG[tag]["B"], 3)))
    seq, lp, _ = _beam(make_model(d, train=False), pg.make_inputs(d, seed=0), int(g["beam_size"]))
    assert np.array_equal(seq[:, 0], g["seq"]), (seq[:, 0], g["seq"])
    np.testing.assert_allclose(lp[:, 0], g["seqLogprobs"], atol=LP_TOL)


# ---- 2. the kernel's own search, judged in float64, over every branch
@pytest.mark.parametrize("name", list(CASES))
def test_own_trace_is_admissible(name):
    dd, W = CASES[name]
    d = pg.make_dims(**dd)
    P, x = pg.make_params(d), pg.make_inputs(d, seed=40 + len(name), ragged=True)
    seq, lp, score, trace = _beam(make_model(d, P, train=False), x, W, return_trace=True)
    _shape_checks(d, W, seq, lp, score, trace)
    checked = cbo.check_admissible(trace, lp, score, seq, P, x, d.L, W)
    assert checked >= d.B * min(d.L, 2)
    for b in range(d.B):                                         # a video's live beams are distinct captions
        live = [tuple(r) for r, s in zip(seq[b], score[b]) if s > cbo.LIVE]
        assert live and len(set(live)) == len(live), b


# ---- 3. W = 1 without suppression is the greedy rollout
@pytest.mark.parametrize("case", ["tiny", "eos"])
def test_width_one_is_the_greedy_rollout(case):
    if case == "tiny":
        g = load_golden("greedy_tiny.npz")
        d = pg.make_dims(**CFG["tiny"])
        P, x = pg.make_params(d, logit_gain=float(g["logit_gain"])), pg.make_inputs(d, seed=0)
    else:
        from tests.util import EOS_CASE
        g = load_golden("greedy_c1_eos.npz")
        d = pg.make_dims(**CFG["c1"])
        P, x = eos_params(d), pg.make_inputs(d, seed=EOS_CASE["input_seed"])
    m = make_model(d, P, train=False)
    seq, lp, score = _beam(m, x, 1, suppress_token=-1)
    with torch.no_grad():
        gs, gl = m.sample(*_inputs(x), {"sample_max": 1})
    gs, gl = gs.cpu().numpy(), gl.cpu().numpy()
    n = gs.shape[1]
    assert np.array_equal(gs, g["seq"])
    assert np.array_equal(seq[:, 0, :n], gs) and (seq[:, 0, n:] == 0).all()
    live = np.concatenate([np.ones((d.B, 1), bool), (gs != 0).cumprod(1).astype(bool)[:, :-1]], 1)      # up to and including the end
    np.testing.assert_allclose(lp[:, 0, :n][live], gl[live], atol=LP_TOL)
    np.testing.assert_allclose(score[:, 0], np.where(live, gl, 0).sum(1), atol=(n + 1) * LP_TOL)


# ---- 4. against the host path on the same model
def test_host_search_on_the_same_model():
    d, P, x, W, g = cbo.load_case("tiny_w3")
    m = make_model(d, P, train=False)
    seq, lp, score = _beam(m, x, W)
    with torch.no_grad():
        hs, hl = m.sample(*_inputs(x), {"beam_size": W})
    assert len(m.done_beams) == d.B
    for b in range(d.B):
        for k, e in enumerate(m.done_beams[b][:W]):
            same = np.array_equal(e["seq"].numpy(), seq[b, k])
            if g["margin"][b] >= cbo.MARGIN:
                assert same, (b, k, e["seq"], seq[b, k])
            if same:
                np.testing.assert_allclose(e["logps"].numpy(), lp[b, k], atol=LP_TOL)
                assert abs(e["p"] - score[b, k]) <= (d.L + 1) * LP_TOL


def test_sample_takes_the_device_search_only_with_its_key(monkeypatch):
    d, P, x, W, g = cbo.load_case("tiny_w3")
    m = make_model(d, P, train=False)
    f = _inputs(x)
    with torch.no_grad():
        seq, lp, _ = m.beam_captions(*f, beam_size=W)
        m.done_beams = marker = ["untouched"]

        def boom(*a, **k):
            raise AssertionError("the host search ran")

        monkeypatch.setattr("controllable_xgating_amd.beam.sample_beam", boom)
        s1, l1 = m.sample(*f, {"beam_size": W, "beam_on_device": True})
        assert m.done_beams is marker
        assert s1.shape == (d.B, d.L) and torch.equal(s1, seq[:, 0]) and torch.equal(l1, lp[:, 0])
        with pytest.raises(AssertionError, match="the host search ran"):
            m.sample(*f, {"beam_size": W})
        with pytest.raises(AssertionError, match="the host search ran"):
            m.sample(*f, {"beam_size": W, "beam_on_device": False})


# ---- 5. the tie rule and the suppression, exactly
def _flat_head(P):
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.full_like(P["logit.bias"], 0.25)
    return P


@pytest.mark.parametrize("suppress", [1, -1])
@pytest.mark.parametrize("V", [61, 20001])
def test_all_equal_logits_follow_the_tie_rule(V, suppress):
    d = pg.make_dims(**dict(CFG["tiny"], B=2, V=V))
    P, x = _flat_head(pg.make_params(d)), pg.make_inputs(d, seed=3)
    seq, lp, score, trace = _beam(make_model(d, P, train=False), x, 3, suppress_token=suppress, return_trace=True)
    o = cbo.beam_captions(P, x, d.L, 3, suppress_token=suppress)
    assert np.array_equal(trace, o["trace"]) and np.array_equal(seq, o["seq"])
    np.testing.assert_allclose(lp, o["seq_logp"], atol=1e-5)
    np.testing.assert_allclose(score[:, 0], -np.log(V), atol=1e-5)


def test_a_dominant_suppressed_word():
    """Word 1 far above every other: never chosen while it is suppressed, chosen first when it is not."""
    d = pg.make_dims(**dict(CFG["tiny"], B=3))
    P, x = pg.make_params(d), pg.make_inputs(d, seed=4)
    P["logit.bias"] = P["logit.bias"].copy()
    P["logit.bias"][1] += np.float32(50.0)
    m = make_model(d, P, train=False)
    seq, lp, score, trace = _beam(m, x, 3, return_trace=True)
    assert not (trace[..., 0] == 1).any() and not (seq == 1).any()
    assert cbo.check_admissible(trace, lp, score, seq, P, x, d.L, 3) >= d.B
    seq, lp, score, trace = _beam(m, x, 3, suppress_token=-1, return_trace=True)
    assert (trace[:, :, 0, 0] == 1).all() and (seq[:, 0] == 1).all()
    np.testing.assert_allclose(lp[:, 0], 0, atol=LP_TOL)


# ---- 6. the workspace and the trace
def test_result_does_not_depend_on_the_workspace_or_the_trace():
    d, P, x, W, g = cbo.load_case("tiny_w3")
    m = make_model(d, P, train=False)
    first = _beam(m, x, W, return_trace=True)
    again = _beam(m, x, W, return_trace=True)
    (key, ws), = m._beam_ws.items()
    m._beam_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}      # NaNs and -1s, and larger
    dirty = _beam(m, x, W, return_trace=True)
    plain = _beam(m, x, W)
    for a, b_, c in zip(first, again, dirty):
        assert np.array_equal(a, b_) and np.array_equal(a, c)
    assert len(plain) == 3 and all(np.array_equal(a, b_) for a, b_ in zip(first, plain))


# ---- 7. into the two-stage captioner
def test_caption_beam_passes_the_device_search_through():
    from controllable_xgating_amd import caption_beam
    from tests import pos_oracle as po
    from tests.pos_control_oracle import cuda_inputs, pos_model
    dp = po.make_dims(**po.POS_CFG["mid"])
    dc = pg.make_dims(**CFG["mid"])
    Wt, W = 2, 3
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    pm = pos_model(dp, P, run)
    cap = make_model(dc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, slp, tm, score = caption_beam(pm, cap, fr, fo, fm, beam_size=Wt, opt={"beam_size": W, "beam_on_device": True})
    assert seq.shape == (dp.B, Wt, dc.L) and slp.shape == seq.shape
    with torch.no_grad():
        _, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
        s2, l2, _ = cap.beam_captions(fr.repeat_interleave(Wt, 0), fo.repeat_interleave(Wt, 0), fm.repeat_interleave(Wt, 0), pos_feats,
                                      beam_size=W)
    assert torch.equal(seq.reshape(dp.B * Wt, -1), s2[:, 0]) and torch.equal(slp.reshape(dp.B * Wt, -1), l2[:, 0])
