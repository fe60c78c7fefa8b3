"""The captioner's beam search under S POS templates per video on the MI355X: SAModel.beam_captions_per_video
(include/xgate_beam_control.h) judged as the search of include/xgate_beam.h on the REPEATED batch -- video b S times, pos_feats row
b S + s -- built in numpy, with the outputs viewed as (B S, ...).  The oracles are tests/cap_beam_oracle.py and its
check_admissible (a float64 replay of the KERNEL'S OWN trace, every group, none excused); then the reference's fixtures at S = 1, the
tie rule and the suppression exactly (the threshold selection's fallback and its candidate list), SAModel.beam_captions on
repeat_interleave'd inputs where the float64 margin pins the tokens, that templates steer and their position does not, workspace and
trace independence, and control.beam_captions_with_templates against the chain done by hand.

Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4.
Pinned groups (float64 margin >= 1e-3), fixed on the CPU by the seeds and gains below: tiny (S 3, W 3) 15 of 15, mid (S 4, W 5)
44 of 48, the control chain 14 of 15."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_beam_oracle as cbo
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
LP_TOL = cbo.LP_TOL

# name -> (dims, S, W): the smallest shapes that reach each branch of the group attention (groups of 4 rows of a video's S W), of
# the step's tiers and of the threshold selection (1024 threads: V against the workgroup, the LDS forms)
CASES = {
    "tiny_s1w1": (CFG["tiny"], 1, 1),                           # one row per video: less than an attention group of 4
    "tiny_s2w2": (CFG["tiny"], 2, 2),                           # exactly one group
    "tiny_s3w3": (CFG["tiny"], 3, 3),                           # two groups plus a row
    "tiny_s3w5": (CFG["tiny"], 3, 5),
    "tiny_s2w8": (CFG["tiny"], 2, 8),                           # a full wave of 64 candidates per (video, template)
    "odd_s2w3": (CFG["odd"], 2, 3),                             # A = 37, R = 20: the rows attention kernel, the unpacked step; V = 37
    "one_s2w2": (CFG["one"], 2, 2),                             # L = 1, K = 1, V = 5
    "mid_s4w5": (CFG["mid"], 4, 5),                             # the packed step (tokens by index)
    "mid_rows_160": (dict(CFG["mid"], B=5), 4, 8),              # past 128 rows
    "v1030": (dict(CFG["tiny"], B=2, V=1030), 2, 3),            # six threads hold two elements, the others one
    "v4100": (dict(CFG["tiny"], B=2, V=4100), 2, 3),
    "v20001": (dict(CFG["tiny"], B=2, V=20001), 2, 3),          # 80 KB of LDS: the opt-in; V % 4 = 1
    "v38500": (dict(CFG["tiny"], B=2, V=38500), 2, 3),          # past 150 KiB: the unstaged form
    "w_equals_v": (dict(CFG["tiny"], B=3, V=8), 2, 8),          # W = V: every word is a candidate, 1016 threads hold nothing
    "c1_s2w5": (dict(CFG["c1"], B=2), 2, 5),                    # the real layer sizes
}
G_ATT, TPB, TW_CAND = 4, 1024, 32                               # rows per attention workgroup; the selection's threads and list capacity


def test_cases_reach_the_branches_they_name():
    for name, (d, S, W) in CASES.items():
        assert S >= 1 and 1 <= W <= min(8, d["V"]), name
    rows = lambda n: CASES[n][1] * CASES[n][2]                                                       # noqa: E731  (per video)
    assert rows("tiny_s1w1") == 1 < G_ATT and rows("tiny_s2w2") == G_ATT and rows("tiny_s3w3") == 2 * G_ATT + 1
    assert CASES["tiny_s2w8"][2] ** 2 == 64
    o = CASES["odd_s2w3"][0]
    assert o["A"] % 4 and o["R"] % 8 and o["V"] == 37
    assert CASES["one_s2w2"][0]["L"] == 1 and CASES["one_s2w2"][0]["K"] == 1 and CASES["one_s2w2"][0]["V"] == 5
    assert all(CASES["mid_s4w5"][0][k] % m == 0 for k, m in (("R", 8), ("E", 4), ("A", 4)))
    assert not CASES["tiny_s3w3"][0]["R"] % 8 and CASES["tiny_s3w3"][0]["E"] % 4 and CASES["tiny_s3w3"][0]["V"] < TPB
    d, S, W = CASES["mid_rows_160"]
    assert d["B"] * S * W == 160 > 128
    assert TPB < CASES["v1030"][0]["V"] < 2 * TPB and CASES["v1030"][0]["V"] - TPB < TPB // 2
    assert 4 * (CASES["v4100"][0]["V"] + 8) <= 64 * 1024 and CASES["v4100"][0]["V"] > 4 * TPB
    assert 64 * 1024 < 4 * (CASES["v20001"][0]["V"] + 8) <= 150 * 1024 and CASES["v20001"][0]["V"] % 4 == 1
    assert 4 * (CASES["v38500"][0]["V"] + 8) > 150 * 1024
    assert CASES["w_equals_v"][2] == CASES["w_equals_v"][0]["V"] == 8
    for n in ("v1030", "v4100", "v20001", "v38500"):
        assert (CASES[n][0]["B"], CASES[n][1], CASES[n][2]) == (2, 2, 3)
    assert (CASES["c1_s2w5"][0]["B"], CASES["c1_s2w5"][0]["V"], CASES["c1_s2w5"][0]["R"]) == (2, 20000, 512)


# ---- inputs: the B videos once, S pos_feats rows each; and the same as the repeated batch
def make_pos(d, S, seed):
    """(B,S,R) float32: S different POS vectors per video."""
    return np.stack([pg.make_inputs(d, seed=seed + 101 * (s + 1))["pos_feats"] for s in range(S)], 1)


def repeated(x, pos):
    """The numpy batch in which video b is repeated S times, with pos_feats row b S + s."""
    S = pos.shape[1]
    xr = {k: np.repeat(v, S, 0) for k, v in x.items()}
    xr["pos_feats"] = np.ascontiguousarray(pos.reshape(-1, pos.shape[2]))
    return xr


def _videos(x):
    return tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))


def _search(m, x, pos, W, **kw):
    """beam_captions_per_video, as numpy viewed over the G = B S groups: [seq (G,W,L), seq_logp, score (G,W)[, trace (G,L,W,2)]]."""
    B, S = pos.shape[:2]
    with torch.no_grad():
        out = m.beam_captions_per_video(*_videos(x), torch.from_numpy(pos).cuda(), beam_size=W, **kw)
    torch.cuda.synchronize()
    assert out[0].shape[:3] == (B, S, W) and out[2].shape == (B, S, W)
    return [v.cpu().numpy().reshape((B * S,) + tuple(v.shape[2:])) for v in out]


def _shape_checks(G, d, W, seq, lp, score, trace):
    assert seq.shape == (G, W, d.L) and seq.dtype == np.int64 and lp.shape == seq.shape and score.shape == (G, W)
    assert trace.shape == (G, d.L, W, 2) and trace.dtype == np.int32
    assert seq.min() >= 0 and seq.max() < d.V and trace[..., 0].min() >= 0 and trace[..., 0].max() < d.V
    assert (score[:, :-1] >= score[:, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()


# ---- 1. the reference's fixtures at S = 1
@pytest.mark.parametrize("name", ["tiny_w3", "eos_w3", "mideos_w5"])
def test_against_the_reference_fixtures_at_one_template(name):
    d, P, x, W, g = cbo.load_case(name)
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, x["pos_feats"][:, None], W, return_trace=True)
    _shape_checks(d.B, d, W, seq, lp, score, trace)
    ok = np.flatnonzero(g["margin"] >= cbo.MARGIN)
    print("%s: %d of %d videos pinned" % (name, len(ok), d.B))
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
    assert cbo.check_admissible(trace, lp, score, seq, P, x, d.L, W) >= d.B       # every video, whatever its margin


# ---- 2. the kernel's own search, judged in float64 on every group, over every branch
@pytest.mark.parametrize("name", list(CASES))
def test_own_trace_is_admissible(name):
    dd, S, W = CASES[name]
    d = pg.make_dims(**dd)
    P, x = pg.make_params(d), pg.make_inputs(d, seed=40 + len(name), ragged=True)
    pos = make_pos(d, S, 7)
    G = d.B * S
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, W, return_trace=True)
    _shape_checks(G, d, W, seq, lp, score, trace)
    checked = cbo.check_admissible(trace, lp, score, seq, P, repeated(x, pos), d.L, W)
    assert checked >= G * min(d.L, 2)
    for g in range(G):                                           # a group's live beams are distinct captions
        live = [tuple(r) for r, s in zip(seq[g], score[g]) if s > cbo.LIVE]
        assert live and len(set(live)) == len(live), g


# ---- 3. the tie rule, exactly
def _flat_head(P):
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.full_like(P["logit.bias"], 0.25)
    return P


@pytest.mark.parametrize("suppress", [1, -1])
@pytest.mark.parametrize("V", [61, 20001])
def test_all_equal_logits_follow_the_tie_rule(V, suppress):
    """Every word ties at the threshold: more candidates than the list holds, the whole workgroup takes the insertion path."""
    d = pg.make_dims(**dict(CFG["tiny"], B=2, V=V))
    S, W = 2, 3
    P, x, pos = _flat_head(pg.make_params(d)), pg.make_inputs(d, seed=3), make_pos(d, S, 5)
    assert V - 1 > TW_CAND
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, W, suppress_token=suppress, return_trace=True)
    o = cbo.beam_captions(P, repeated(x, pos), d.L, W, suppress_token=suppress)
    assert np.array_equal(trace, o["trace"]) and np.array_equal(seq, o["seq"])
    np.testing.assert_allclose(lp, o["seq_logp"], atol=1e-5)
    np.testing.assert_allclose(score[:, 0], -np.log(V), atol=1e-5)


def test_ten_words_tie_inside_the_candidate_list():
    """Ten words share the largest bias, the rest lie lower: tau is the tied value, the list holds exactly the ten (no overflow),
    and the lowest three indices win at every step and slot."""
    d = pg.make_dims(**dict(CFG["tiny"], B=2, V=4100))
    S, W = 2, 3
    P, x, pos = _flat_head(pg.make_params(d)), pg.make_inputs(d, seed=3), make_pos(d, S, 5)
    assert W < 10 <= TW_CAND
    top = np.array([9, 700, 1023, 1024, 1025, 2047, 2048, 3000, 4098, 4099])     # several share a thread (i and i + 1024 k)
    P["logit.bias"] = P["logit.bias"].copy()
    P["logit.bias"][top] = np.float32(3.25)
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, W, return_trace=True)
    o = cbo.beam_captions(P, repeated(x, pos), d.L, W)
    assert np.array_equal(trace, o["trace"]) and np.array_equal(seq, o["seq"])
    assert set(np.unique(trace[..., 0]).tolist()) == set(top[:3].tolist())
    assert (trace[:, 0, :, 0] == top[:3]).all()
    np.testing.assert_allclose(lp, o["seq_logp"], atol=1e-5)


# ---- 4. a dominant suppressed word
def test_a_dominant_suppressed_word():
    """Word 1 far above every other: never chosen while it is suppressed, chosen first when it is not."""
    d = pg.make_dims(**dict(CFG["tiny"], B=3))
    S, W = 2, 3
    P, x, pos = pg.make_params(d), pg.make_inputs(d, seed=4), make_pos(d, S, 9)
    P["logit.bias"] = P["logit.bias"].copy()
    P["logit.bias"][1] += np.float32(50.0)
    m = make_model(d, P, train=False)
    seq, lp, score, trace = _search(m, x, pos, W, return_trace=True)
    assert not (trace[..., 0] == 1).any() and not (seq == 1).any()
    assert cbo.check_admissible(trace, lp, score, seq, P, repeated(x, pos), d.L, W) >= d.B * S
    seq, lp, score, trace = _search(m, x, pos, W, suppress_token=-1, return_trace=True)
    assert (trace[:, :, 0, 0] == 1).all() and (seq[:, 0] == 1).all()
    np.testing.assert_allclose(lp[:, 0], 0, atol=LP_TOL)


# ---- 5. against beam_captions on repeat_interleave'd inputs
# name -> (CFG entry, S, W, input seed, logit_gain): seed and gain chosen on the CPU so that the float64 oracle ALONE pins at least
# four fifths of the groups (the margin as tools/gen_cap_beam_golden.py derives it: VideoSearch.margin over the steps that select
# a live candidate)
PINNED = {"tiny": ("tiny", 3, 3, 1, 32.0), "mid": ("mid", 4, 5, 2, 128.0)}


@functools.lru_cache(maxsize=None)
def _pinned_case(name):
    cfg, S, W, seed, gain = PINNED[name]
    d = pg.make_dims(**CFG[cfg])
    P, x = pg.make_params(d, logit_gain=gain), pg.make_inputs(d, seed=seed)
    pos = make_pos(d, S, seed)
    torch.set_num_threads(8)
    margin = cbo.beam_captions(P, repeated(x, pos), d.L, W, dtype=torch.float64)["margin"]
    return d, P, x, pos, W, margin


def _assert_pinned_groups_agree(margin, got, want, L):
    ok = np.flatnonzero(margin >= cbo.MARGIN)
    print("%d of %d groups pinned" % (len(ok), len(margin)))
    assert 5 * len(ok) >= 4 * len(margin)                        # a condition on the inputs, not a measurement
    (seq, lp, score), (seq_r, lp_r, score_r) = got, want
    assert np.array_equal(seq[ok], seq_r[ok]), np.flatnonzero((seq[ok] != seq_r[ok]).any((1, 2)))
    np.testing.assert_allclose(lp[ok], lp_r[ok], atol=LP_TOL)
    np.testing.assert_allclose(score[ok], score_r[ok], atol=(L + 1) * LP_TOL)


@pytest.mark.parametrize("name", list(PINNED))
def test_against_beam_captions_on_repeated_inputs(name):
    d, P, x, pos, W, margin = _pinned_case(name)
    S = pos.shape[1]
    m = make_model(d, P, train=False)
    got = _search(m, x, pos, W)
    with torch.no_grad():
        want = m.beam_captions(*(t.repeat_interleave(S, 0) for t in _videos(x)), torch.from_numpy(pos).cuda().reshape(d.B * S, -1),
                               beam_size=W)
    _assert_pinned_groups_agree(margin, got, [v.cpu().numpy() for v in want], d.L)


# ---- 6. templates steer, and their position does not
def test_templates_steer_and_their_position_does_not():
    d = pg.make_dims(**CFG["mid"])
    S, W = 3, 3
    P, x, pos = pg.make_params(d), pg.make_inputs(d, seed=6), make_pos(d, S, 6)
    m = make_model(d, P, train=False)
    pos_same = pos.copy()
    pos_same[:, 2] = pos_same[:, 0]
    out = [v.reshape((d.B, S) + v.shape[1:]) for v in _search(m, x, pos_same, W, return_trace=True)]
    for v in out:
        assert np.array_equal(v[:, 0], v[:, 2])                  # bit-equal: a group knows neither s nor its place in an attention group
    seq = _search(m, x, pos, W)[0].reshape(d.B, S, W, d.L)
    assert any(not np.array_equal(seq[b, 0, 0], seq[b, 1, 0]) or not np.array_equal(seq[b, 0, 0], seq[b, 2, 0]) for b in range(d.B))


# ---- 7. the workspace and the trace
def test_result_does_not_depend_on_the_workspace_or_the_trace():
    d, P, x, W, g = cbo.load_case("tiny_w3")
    pos = make_pos(d, 3, 1)
    m = make_model(d, P, train=False)
    first = _search(m, x, pos, W, return_trace=True)
    again = _search(m, x, pos, W, return_trace=True)
    (key, ws), = m._beam_control_ws.items()
    m._beam_control_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}   # NaNs and -1s, and larger
    dirty = _search(m, x, pos, W, return_trace=True)
    plain = _search(m, x, pos, W)
    for a, b_, c in zip(first, again, dirty):
        assert np.array_equal(a, b_) and np.array_equal(a, c)
    assert len(plain) == 3 and all(np.array_equal(a, b_) for a, b_ in zip(first, plain))


# ---- 8. through the control chain
CHAIN = dict(S=3, W=3, input_seed=20, template_seed=11, logit_gain=32.0)       # chosen on the CPU like PINNED


@functools.lru_cache(maxsize=None)
def chain_case():
    """The tiny POS generator in front of the tiny captioner: (dp, dc, POS params, running, inputs, templates, captioner params,
    float64 margins of the repeated batch under the POS ORACLE's pos_feats)."""
    from tests import pos_control_oracle as pco
    from tests import pos_oracle as po
    dp, dc = po.make_dims(**po.POS_CFG["tiny"]), pg.make_dims(**CFG["tiny"])
    assert (dp.B, dp.K, dp.R, dp.F1, dp.F2) == (dc.B, dc.K, dc.R, dc.F1, dc.F2)
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=CHAIN["input_seed"], ragged=True)
    tm, _ = pco.seeded_templates(dp.B, CHAIN["S"], dp.L, dp.C, seed=CHAIN["template_seed"])
    Pc = pg.make_params(dc, logit_gain=CHAIN["logit_gain"])
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    o = pco.sample_forced(po.to_torch(P), po.to_torch(run), fr, fo, fm, tm, dp.L)
    xr = repeated({k: x[k] for k in ("feats_rgb", "feats_opfl", "feat_mask")}, o["pos_feats"].numpy().reshape(dp.B, CHAIN["S"], -1))
    torch.set_num_threads(8)
    margin = cbo.beam_captions(Pc, xr, dc.L, CHAIN["W"], dtype=torch.float64)["margin"]
    return dp, dc, P, run, x, tm, Pc, margin


def test_beam_captions_with_templates_is_the_chain_done_by_hand():
    from controllable_xgating_amd import beam_captions_with_templates
    from tests.pos_control_oracle import cuda_inputs, pos_model
    dp, dc, P, run, x, tm, Pc, margin = chain_case()
    S, W = CHAIN["S"], CHAIN["W"]
    G = dp.B * S
    pm, cap = pos_model(dp, P, run), make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, lp, score, tscore = beam_captions_with_templates(pm, cap, fr, fo, fm, tm, beam_size=W)
    assert seq.shape == (dp.B, S, W, dc.L) and lp.shape == seq.shape and score.shape == (dp.B, S, W) and tscore.shape == (dp.B, S)
    assert not any(t.requires_grad for t in (seq, lp, score, tscore))
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
        want = cap.beam_captions(fr.repeat_interleave(S, 0), fo.repeat_interleave(S, 0), fm.repeat_interleave(S, 0), pos_feats,
                                 beam_size=W)
    assert torch.equal(tscore, tag_logp.sum(2))
    got = [v.cpu().numpy().reshape((G,) + tuple(v.shape[2:])) for v in (seq, lp, score)]
    _assert_pinned_groups_agree(margin, got, [v.cpu().numpy() for v in want], dc.L)
