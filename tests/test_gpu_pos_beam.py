"""POS beam search on the MI355X: PosModel.beam_templates (include/xgate_pos_beam.h) against the reference's fixtures
tests/golden/pos_beam_*.npz where their selection margins pin the tokens, and everywhere -- no row excused -- by
tests/pos_beam_oracle.check_admissible: a float64 replay (eager torch on the same GPU) of the KERNEL'S OWN (token, parent) trace
that asserts every selection was a legal one within the rounding of the numbers it was made from.  Then consistency with the
forced and the greedy calls, the tie rule in both head forms, determinism and workspace independence, and control.caption_beam.

Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import pos_beam_oracle as pbo
from tests import pos_oracle as po
from tests.pos_control_oracle import cuda_inputs, pos_model
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
F64 = torch.float64
LP_TOL = pbo.LP_TOL
GROUP = 4                                   # XGPC_TEMPLATE_GROUP

# name -> (dims, W): the smallest shapes that reach each branch of pos_beam_merge_kernel and of the launches around it
SMALL = dict(E=18, C=5, L=6, F1=20, F2=12)
HEAD = dict(B=2, K=5, R=40, A=52, E=24, L=6, F1=20, F2=12)
CASES = {
    "tiny_w1": (po.POS_CFG["tiny"], 1),                                             # pos_attn_kernel; one candidate row
    "tiny_w3": (po.POS_CFG["tiny"], 3),
    "tiny_w5": (po.POS_CFG["tiny"], 5),                                             # W = C: the suppressed tag is a candidate
    "a_r_odd": (dict(B=3, K=5, R=22, A=38, **SMALL), 3),                            # A % 4 != 0 (scalar loads), R % 4 != 0
    "mid_w5": (po.POS_CFG["mid"], 5),                                               # a full attention group and a partial one
    "mid_w8": (po.POS_CFG["mid"], 8),                                               # a full wave of 64 candidates
    "c64": (dict(HEAD, C=64), 4),                                                   # the last size of the lane-per-category merge
    "c65": (dict(HEAD, C=65), 4),                                                   # the first size of the serial one
    "c130": (dict(HEAD, C=130), 4),
    "k_past_prefetch": (dict(B=2, K=300, R=64, A=96, E=36, C=20, L=6, F1=48, F2=40), 3),   # ceil(K / nsplit) = 19 > 16 registers
    "rows_300": (dict(po.POS_CFG["mid"], B=100), 3),                                # > 256 rows: n_out, the backtrace, the products
    "wide_a": (dict(B=2, K=5, R=24, A=3300, E=18, C=5, L=4, F1=20, F2=12), 3),      # the one-template attention form
    "c1_w5": (po.POS_CFG["c1"], 5),                                                 # the real layer sizes
    "full64_w5": (po.POS_CFG["full64"], 5),
}


def test_cases_reach_the_branches_they_name():
    def group_lds(d, G):                                         # xg_pos.hip: attn_group_lds
        nsplit = min(max(1024 // d["R"], 1), d["K"])
        r4 = lambda v: (v + 3) // 4 * 4                          # noqa: E731
        return 4 * (r4(G * max(d["A"], nsplit * d["R"])) + r4(d["A"]) + G * d["K"])

    for name, (d, W) in CASES.items():
        assert 1 <= W <= min(8, d["C"]) and 4 * W * (2 * d["R"] + d["C"]) + 1024 <= 65536, name
        assert (group_lds(d, GROUP) > 64 * 1024) == (name == "wide_a") and group_lds(d, 1) <= 64 * 1024, name
    assert CASES["tiny_w5"][1] == CASES["tiny_w5"][0]["C"]
    d, W = CASES["a_r_odd"]
    assert d["A"] % 4 and d["R"] % 4
    assert CASES["mid_w5"][1] % GROUP == 1 and CASES["mid_w8"][1] ** 2 == 64
    assert [CASES[k][0]["C"] for k in ("c64", "c65", "c130")] == [64, 65, 130]
    d, W = CASES["k_past_prefetch"]
    assert -(-d["K"] // min(max(1024 // d["R"], 1), d["K"])) > 16
    d, W = CASES["rows_300"]
    assert d["B"] * W == 300


def _beam(m, x, W, **kw):
    with torch.no_grad():
        out = m.beam_templates(*cuda_inputs(x), beam_size=W, **kw)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in out]


def _f64(P, run, x):
    Pt, rt = po.to_torch(P, F64, "cuda"), po.to_torch(run, F64, "cuda")
    return Pt, rt, [torch.from_numpy(x[k]).to("cuda", F64) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


def _admissible(d, P, run, x, W, suppress, tm, lp, score, trace):
    Pt, rt, f = _f64(P, run, x)
    return pbo.check_admissible(trace, lp, score, tm, lambda tr: pbo.logps_along_trace(Pt, rt, *f, tr),
                                C=d.C, L=d.L, W=W, suppress_tag=suppress)


def _shape_checks(d, W, tm, lp, score, mk, trace):
    assert tm.shape == (d.B, W, d.L) and tm.dtype == np.int64 and lp.shape == tm.shape and score.shape == (d.B, W)
    assert mk.shape == (d.B, W, d.L + 1) and trace.shape == (d.B, d.L, W, 2) and trace.dtype == np.int32
    assert tm.min() >= 0 and tm.max() < d.C
    assert np.array_equal(mk, pbo.masks_of(tm).astype(np.float32))
    assert (score[:, :-1] >= score[:, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()


# ---- 1. against the reference's fixtures
@pytest.mark.parametrize("name", list(pbo.BEAM_CASES))
def test_against_the_reference_fixtures(name):
    d, P, run, x, W, g = pbo.load_case(name)
    tm, lp, score, mk, trace = _beam(pos_model(d, P, run), x, W, trim=False, return_trace=True)
    _shape_checks(d, W, tm, lp, score, mk, trace)
    ok = np.flatnonzero(g["margin"] >= pbo.MARGIN)
    print("%s: margins %s -> %d of %d videos pinned" % (name, " ".join("%.1e" % v for v in g["margin"]), len(ok), d.B))
    if name.startswith("tiny"):
        assert len(ok) == d.B                                    # conditions of the fixtures, not measurements
    if name == "eos_w3":
        assert len(ok) >= 5
    n = min(d.L, int((tm != 0).cumprod(2).sum(2).max()))
    for b in ok:
        assert np.array_equal(trace[b, :, :, 0], g["tokens"][b]), (b, trace[b, :, :, 0], g["tokens"][b])
        vs = pbo.VideoSearch(W, d.L, np.float32)                 # steps 3-5 over the reference's own log-probabilities
        for t in range(d.L):
            s = g["logps"][b, t].copy()
            s[:, 1] -= np.float32(1000)
            vs.feed(s)
        assert np.array_equal(trace[b], vs.trace), b
        ranked = vs.result()
        assert np.array_equal(tm[b], np.array([e["seq"] for e in ranked])), b
        np.testing.assert_allclose(lp[b], np.array([e["logps"] for e in ranked]), atol=LP_TOL)
        np.testing.assert_allclose(score[b], np.array([e["score"] for e in ranked]), atol=(n + 1) * LP_TOL)
    if name == "tiny_w5":                                        # W = C: category 1 among the candidates, a best beam ending at once
        assert (trace[:, 0, :, 0] == 1).any(1).all() and (tm[:, 0] == 0).all(1).any()
    # every video, whatever its margin
    assert _admissible(d, P, run, x, W, 1, tm, lp, score, trace) >= d.B


# ---- 2. the kernel's own search, judged in float64, over every branch
@pytest.mark.parametrize("name", list(CASES))
def test_own_trace_is_admissible(name):
    dd, W = CASES[name]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=40 + len(name), ragged=True)
    tm, lp, score, mk, trace = _beam(pos_model(d, P, run), x, W, trim=False, return_trace=True)
    _shape_checks(d, W, tm, lp, score, mk, trace)
    checked = _admissible(d, P, run, x, W, 1, tm, lp, score, trace)
    assert checked >= d.B * 2
    for b in range(d.B):                                         # a video's live beams are distinct templates
        live = [tuple(r) for r, s in zip(tm[b], score[b]) if s > pbo.LIVE]
        assert live and len(set(live)) == len(live), b


# ---- 3. consistency with the merged calls
@pytest.mark.parametrize("name", ["tiny_w5", "mid_w8", "c1_w5"])
def test_forced_call_on_the_beams_scores_them_alike(name):
    dd, W = CASES[name]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    with torch.no_grad():
        tm, lp, score, mk = m.beam_templates(*cuda_inputs(x), beam_size=W)
        lp_f, _, mk_f, _ = m.sample_forced(*cuda_inputs(x), tm, collect_states=False)
    n = tm.shape[2]
    assert lp_f.shape == lp.shape and torch.equal(mk, mk_f)
    lp, lp_f, score = lp.cpu().numpy(), lp_f.cpu().numpy(), score.cpu().numpy()
    live = lp > pbo.LIVE
    assert live.any()
    np.testing.assert_allclose(lp_f[live], lp[live], atol=LP_TOL)
    rows = score > pbo.LIVE                                      # a beam that holds no suppressed tag: its score is the template's
    assert rows[:, 0].all()
    np.testing.assert_allclose(lp_f.sum(2)[rows], score[rows], atol=(n + 1) * LP_TOL)


@pytest.mark.parametrize("name", ["tiny", "eos"])
def test_width_one_without_suppression_is_the_greedy_rollout(name):
    from tests.pos_control_oracle import load_case
    d, P, run, x, _ = load_case(name)
    m = pos_model(d, P, run)
    with torch.no_grad():
        seq, slp, _, mk_g = m.sample(*cuda_inputs(x), {"sample_max": 1})
        tm, lp, score, mk = m.beam_templates(*cuda_inputs(x), beam_size=1, suppress_tag=-1, trim=False)
    n = seq.shape[1]
    assert n >= 1 and torch.equal(tm[:, 0, :n], seq) and int(tm[:, 0, n:].abs().sum()) == 0
    assert torch.equal(mk[:, 0, :n + 1], mk_g)
    alive = mk[:, 0, :n].bool()                                  # up to and including each row's end tag
    np.testing.assert_allclose(lp[:, 0, :n][alive].cpu().numpy(), slp[alive].cpu().numpy(), atol=LP_TOL)


# ---- 4. the tie rule, in both head forms
@pytest.mark.parametrize("Cn", [5, 70])
def test_all_equal_logits_follow_the_tie_rule(Cn):
    from tests.test_pos_beam_cpu import TIE_TRACE, _flat_head
    d = po.make_dims(**dict(po.POS_CFG["tiny"], B=2, C=Cn))
    P, run, x = _flat_head(d, po.make_params(d)), po.make_running(d), po.make_inputs(d, seed=3)
    o = pbo.beam_templates(po.to_torch(P), po.to_torch(run), *[torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask")],
                           d.L, 3)
    tm, lp, score, mk, trace = _beam(pos_model(d, P, run), x, 3, trim=False, return_trace=True)
    assert [[tuple(v) for v in step] for step in trace[0, :2].tolist()] == TIE_TRACE[1]
    assert np.array_equal(trace, o["trace"]) and np.array_equal(tm, o["templates"]) and np.array_equal(mk, o["masks"])
    np.testing.assert_allclose(lp, o["tag_logp"], atol=LP_TOL)
    np.testing.assert_allclose(score, o["score"], atol=(d.L + 1) * LP_TOL)


# ---- 5. determinism, the workspace, the optional outputs
def test_two_calls_and_a_poisoned_workspace_give_the_same_bits():
    dd, W = CASES["mid_w5"]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    a, b = _beam(m, x, W, trim=False, return_trace=True), _beam(m, x, W, trim=False, return_trace=True)
    for v, w in zip(a, b):
        assert np.array_equal(v, w)
    _beam(m, x, 8, trim=False)                                   # a wider beam: a larger workspace
    ws = m._cws
    n_big = ws.numel()
    ws[:n_big // 4 * 4].view(torch.float32).fill_(float("nan"))
    c = _beam(m, x, W, trim=False, return_trace=True)
    assert m._cws is ws and ws.numel() == n_big                  # the same, larger, poisoned workspace served the call
    for v, w in zip(a, c):
        assert np.array_equal(v, w)
    # without the trace, and trimmed: the same bits
    tm, lp, score, mk = _beam(m, x, W, trim=False)
    assert np.array_equal(tm, a[0]) and np.array_equal(lp, a[1]) and np.array_equal(score, a[2]) and np.array_equal(mk, a[3])
    n = min(d.L, int((tm != 0).cumprod(2).sum(2).max()))
    tm_t, lp_t, score_t, mk_t = _beam(m, x, W)
    assert tm_t.shape == (d.B, W, n) and mk_t.shape == (d.B, W, n + 1)
    assert np.array_equal(tm_t, tm[:, :, :n]) and np.array_equal(lp_t, lp[:, :, :n]) and np.array_equal(mk_t, mk[:, :, :n + 1])
    assert (tm[:, :, n:] == 0).all() and np.array_equal(score_t, score)


def test_an_end_tag_at_once_gives_n_zero():
    d = po.make_dims(**po.POS_CFG["tiny"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5)
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.array([5, 0, 0, 0, 0], np.float32)
    m = pos_model(d, P, run)
    tm, lp, score, mk = _beam(m, x, 1)
    assert tm.shape == (d.B, 1, 0) and lp.shape == (d.B, 1, 0) and mk.shape == (d.B, 1, 1) and (mk == 1).all()
    np.testing.assert_allclose(score, -np.log1p(4 * np.exp(-5.0)), atol=LP_TOL)
    with pytest.raises(ValueError):
        m.beam_templates(*cuda_inputs(x), beam_size=6)            # W > C
    with pytest.raises(ValueError):
        m.beam_templates(*cuda_inputs(x), beam_size=0)
    with pytest.raises(ValueError):
        m.beam_templates(*cuda_inputs(x), beam_size=3, suppress_tag=5)


# ---- 6. into the captioner
def test_caption_beam_is_caption_with_templates_on_the_beams():
    from controllable_xgating_amd import caption_beam, caption_with_templates
    dp = po.make_dims(**po.POS_CFG["mid"])
    dc = pg.make_dims(**CFG["mid"])
    assert (dp.K, dp.R, dp.F1, dp.F2) == (dc.K, dc.R, dc.F1, dc.F2)
    W = 4
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    pm = pos_model(dp, P, run)
    # the POS-weighted captioner of tests/test_gpu_pos_sample.py: its greedy captions move with the POS vector
    Pc = pg.make_params(dc)
    Pc["lstmcore.lstm_1.a2h.weight"] = Pc["lstmcore.lstm_1.a2h.weight"] * np.float32(16.0)
    cap = make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, slp, tm, score = caption_beam(pm, cap, fr, fo, fm, beam_size=W, opt={"sample_max": 1})
    assert not seq.requires_grad and not slp.requires_grad and not score.requires_grad
    assert seq.shape[:2] == (dp.B, W) and slp.shape == seq.shape and tm.shape == (dp.B, W, dp.L) and score.shape == (dp.B, W)
    seq_w, slp_w, _ = caption_with_templates(pm, cap, fr, fo, fm, tm, {"sample_max": 1})
    assert torch.equal(seq, seq_w) and torch.equal(slp, slp_w)
    with torch.no_grad():
        tm2, _, score2, _ = pm.beam_templates(fr, fo, fm, beam_size=W, trim=False)
    assert torch.equal(tm, tm2) and torch.equal(score, score2)
    tn, sn = tm.cpu().numpy(), seq.cpu().numpy()
    apart = [(b, s) for b in range(dp.B) for s in range(1, W)
             if not np.array_equal(tn[b, s], tn[b, 0]) and not np.array_equal(sn[b, s], sn[b, 0])]
    assert apart
