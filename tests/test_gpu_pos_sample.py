"""Sampled POS templates on the MI355X: PosModel.sample_templates (include/xgate_pos_sample.h) against the float64 oracle's own
draw from the same uniforms (tests/pos_sample_oracle.py in eager torch on the same GPU), every row against a float64 replay of
the kernel's own tokens (tests/pos_control_oracle.py) over every branch of pos_cell_head_rows_kernel<true> and the launches around
it, bit for bit against the forced call fed the sampled templates and against the greedy call at a low temperature, at the edge
uniforms, and control.caption_sampled against control.caption_with_templates.

Bounds: those of tests/test_gpu_pos_control.py for this model -- states, pos_feats and masks 1e-4, log-probabilities 3e-4."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import pos_control_oracle as pco
from tests import pos_oracle as po
from tests import pos_sample_oracle as pso
from tests.pos_control_oracle import cuda_inputs, load_case, pos_model
from tests.util import CFG, assert_sampled_tokens_match, make_model

pytestmark = pytest.mark.gpu
F64 = torch.float64
ST_TOL, LP_TOL = 1e-4, 3e-4
EDGE_TOL = 3e-4                             # a draw this close to an edge of the oracle's CDF interval may fall either way
GROUP = 4                                   # XGPC_TEMPLATE_GROUP
FIXTURES = ("tiny", "c1", "ragged", "eos")
TEMPERATURES = (0.7, 1.0, 1.3)

# name -> (dims, S): the smallest shapes at which each branch of pos_cell_head_rows_kernel<true> and of the launches around it can go
# wrong (tests/test_pos_sample_cpu.py: test_replay_cases_reach_the_branches_they_name)
SMALL = dict(E=18, C=5, L=6, F1=20, F2=12)
HEAD = dict(B=2, K=5, R=40, A=52, E=24, L=6, F1=20, F2=12)
CASES = {
    "tiny_s3": (po.POS_CFG["tiny"], 3),                                             # 15 rows, nothing a multiple of 8
    "a_r_odd": (dict(B=3, K=5, R=22, A=38, **SMALL), 2),                            # A % 4 != 0 (scalar loads), R % 4 != 0
    "group_plus_1": (dict(po.POS_CFG["mid"], B=3), GROUP + 1),                      # S = 5: a full group and a partial one
    "c64": (dict(HEAD, C=64), 3),                                                   # the last size of the lane-per-category head
    "c65": (dict(HEAD, C=65), 3),                                                   # the first size of the serial head
    "c130": (dict(HEAD, C=130), 3),                                                 # serial, more than two waves of categories
    "rows_297": (dict(po.POS_CFG["tiny"], B=9), 33),                                # > 256 rows: n_out, the products
    "c1_s8": (po.POS_CFG["c1"], 8),                                                 # the real layer sizes
}


def _uniforms(d, S, seed=11):
    return torch.from_numpy(pg.uniform("pos_sample_u", (d.B, S, d.L), seed))


def _sampled(m, x, S, u, temperature=1.0, **kw):
    with torch.no_grad():
        out = m.sample_templates(*cuda_inputs(x), S, temperature=temperature, uniforms=u, **kw)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in out]


def _f64(P, run, x):
    Pt, rt = po.to_torch(P, F64, "cuda"), po.to_torch(run, F64, "cuda")
    return Pt, rt, [torch.from_numpy(x[k]).to("cuda", F64) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


def _replay(d, P, run, x, tm):
    """The float64 forced oracle on the GPU fed the templates `tm` (numpy): its outputs as numpy."""
    Pt, rt, f = _f64(P, run, x)
    o = pco.sample_forced(Pt, rt, *f, torch.from_numpy(tm), d.L)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()}


# ---- 1. tokens against the oracle's own draw
@functools.lru_cache(maxsize=None)
def _fixture_case(name):
    d, P, run, x, _ = load_case(name)
    return d, P, run, x, _uniforms(d, 5)


@pytest.mark.parametrize("temperature", TEMPERATURES)
@pytest.mark.parametrize("name", FIXTURES)
def test_tokens_match_the_oracles_own_draw(name, temperature):
    d, P, run, x, u = _fixture_case(name)
    S, M = 5, d.B * 5
    Pt, rt, f = _f64(P, run, x)
    o = pso.sample_templates(Pt, rt, *f, u, d.L, temperature)
    tm, lp, _, masks, pf = _sampled(pos_model(d, P, run), x, S, u, temperature, trim=False)
    assert tm.shape == (d.B, S, d.L) and tm.dtype == np.int64 and lp.shape == tm.shape and masks.shape == (d.B, S, d.L + 1)
    assert tm.min() >= 0 and tm.max() < d.C
    u2 = np.zeros((d.L + 1, M), np.float32)                      # the helper's layout: the draw of step t reads u[t, row]
    u2[1:] = u.numpy().reshape(M, d.L).T
    logps = [v.cpu() for v in o["logps"]]
    excused = assert_sampled_tokens_match(tm.reshape(M, d.L), o["templates"].cpu().numpy().reshape(M, d.L), logps, u2,
                                          temperature=temperature, tol=EDGE_TOL)
    print("%s T=%.1f: %d of %d rows excused by the edge rule" % (name, temperature, len(excused), M))
    assert len(excused) * 8 <= M, excused
    keep = np.setdiff1d(np.arange(M), excused)                   # the rows that drew the oracle's tokens follow its rollout
    np.testing.assert_allclose(lp.reshape(M, -1)[keep], o["tag_logp"].cpu().numpy().reshape(M, -1)[keep], atol=LP_TOL)
    np.testing.assert_allclose(pf[keep], o["pos_feats"].cpu().numpy()[keep], atol=ST_TOL)
    assert np.array_equal(masks.reshape(M, -1)[keep], o["masks"].cpu().numpy().reshape(M, -1)[keep])
    for b in range(d.B):                                         # the draws are diverse: >= 2 distinct templates per video
        assert len({tuple(r) for r in tm[b]}) >= 2, b
    assert ((tm > 0).all(2) == False).any()                      # noqa: E712 -- and at least one row ends before L
    alive = np.concatenate([np.ones((d.B, S, 1), bool), np.cumprod(tm[:, :, :-1] > 0, 2).astype(bool)], 2)
    assert (tm[~alive] == 0).all() and (lp[~alive] == 0).all() and (lp[alive] < 0).all()


# ---- 2. every row against a float64 replay of the kernel's own tokens
@pytest.mark.parametrize("name", list(CASES))
def test_every_row_vs_f64_replay_of_its_own_tokens(name):
    dd, S = CASES[name]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=40 + len(name), ragged=True)
    u = _uniforms(d, S, seed=7 + len(name))
    m = pos_model(d, P, run)
    tm, lp, states, masks, pf = _sampled(m, x, S, u, collect_states=True, trim=False)
    assert tm.shape == (d.B, S, d.L) and lp.shape == tm.shape and states.shape == (d.B, S, d.L + 1, d.R)
    assert masks.shape == (d.B, S, d.L + 1) and pf.shape == (d.B * S, d.R)
    assert tm.min() >= 0 and tm.max() < d.C
    alive = np.concatenate([np.ones((d.B, S, 1), bool), np.cumprod(tm[:, :, :-1] > 0, 2).astype(bool)], 2)
    assert (tm[~alive] == 0).all() and (lp[~alive] == 0).all() and (lp[alive] < 0).all()
    assert len({tuple(r) for r in tm.reshape(-1, d.L)}) > 1
    o = _replay(d, P, run, x, tm)
    np.testing.assert_allclose(lp, o["tag_logp"], atol=LP_TOL)
    np.testing.assert_allclose(states, o["states"], atol=ST_TOL)
    assert np.array_equal(masks, o["masks"])
    np.testing.assert_allclose(pf, o["pos_feats"], atol=ST_TOL)
    np.testing.assert_allclose(lp.sum(2), o["tag_logp"].sum(2), atol=LP_TOL * d.L)
    assert np.array_equal(pf.reshape(d.B, S, d.R), states[:, :, d.L])
    # trimmed to the reference's n, and without the states: the same bits
    n = o["n"]
    tm_t, lp_t, st_t, mk_t, pf_t = _sampled(m, x, S, u)
    assert st_t is None and tm_t.shape == (d.B, S, n)
    assert np.array_equal(tm_t, tm[:, :, :n]) and np.array_equal(lp_t, lp[:, :, :n]) and np.array_equal(mk_t, masks[:, :, :n + 1])
    assert np.array_equal(pf_t, pf) and (tm[:, :, n:] == 0).all()


# ---- 3. bit identity with the forced call
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("cfg", ["tiny", "c1"])
def test_forced_call_on_the_sampled_templates_gives_the_same_bits(cfg, S):
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    with torch.no_grad():
        tm, lp, st, mk, pf = m.sample_templates(*cuda_inputs(x), S, uniforms=_uniforms(d, S, seed=3), collect_states=True, trim=False)
        lp_f, st_f, mk_f, pf_f = m.sample_forced(*cuda_inputs(x), tm, trim=False)
    assert int((tm > 0).sum()) > 0
    assert torch.equal(st, st_f) and torch.equal(mk, mk_f) and torch.equal(pf, pf_f) and torch.equal(lp, lp_f)


# ---- 4. a low temperature is the greedy rollout
@pytest.mark.parametrize("name", ["c1", "eos"])
def test_low_temperature_has_the_bits_of_greedy(name):
    d, P, run, x, _ = load_case(name)
    m = pos_model(d, P, run)
    with torch.no_grad():
        seq, _, st_g, mk_g = m.sample(*cuda_inputs(x), {"sample_max": 1})
        tm, _, st, mk, pf = m.sample_templates(*cuda_inputs(x), 1, temperature=1e-5, uniforms=torch.full((d.B, 1, d.L), 0.5),
                                               collect_states=True)
    n = seq.shape[1]
    assert n >= 1 and tm.shape == (d.B, 1, n)
    assert torch.equal(tm[:, 0], seq) and torch.equal(st[:, 0], st_g) and torch.equal(mk[:, 0], mk_g)
    assert torch.equal(pf, st_g[:, n])


# ---- 5. edge uniforms, in both head forms
@pytest.mark.parametrize("Cn", [5, 130])
def test_edge_uniforms(Cn):
    d = po.make_dims(**dict(HEAD, C=Cn))
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=9, ragged=True)
    m = pos_model(d, P, run)
    S = 3
    with torch.no_grad():
        tm, lp, st, mk, pf = m.sample_templates(*cuda_inputs(x), S, uniforms=torch.zeros(d.B, S, d.L), collect_states=True)
        lp_f, st_f, mk_f, pf_f = m.sample_forced(*cuda_inputs(x), torch.zeros(d.B, S, d.L, dtype=torch.int64))
        assert tm.shape == (d.B, S, 0) and mk.shape == (d.B, S, 1) and st.shape == (d.B, S, 1, d.R)           # n = 0
        assert torch.equal(pf, pf_f) and torch.equal(st, st_f) and torch.equal(mk, mk_f)
        tm0, lp0, _, mk0, _ = m.sample_templates(*cuda_inputs(x), S, uniforms=torch.zeros(d.B, S, d.L), trim=False)
        assert int(tm0.abs().sum()) == 0 and bool((lp0[:, :, 0] < 0).all()) and bool((lp0[:, :, 1:] == 0).all())
        assert bool((mk0[:, :, 0] == 1).all()) and bool((mk0[:, :, 1:] == 0).all())
        tm, lp, st, mk, pf = m.sample_templates(*cuda_inputs(x), S, uniforms=torch.ones(d.B, S, d.L), collect_states=True)
        assert tm.shape == (d.B, S, d.L) and bool((tm == Cn - 1).all())                                      # n = L
        lp_f, st_f, mk_f, pf_f = m.sample_forced(*cuda_inputs(x), tm)
        assert torch.equal(pf, pf_f) and torch.equal(st, st_f) and torch.equal(mk, mk_f) and torch.equal(lp, lp_f)
        assert bool((mk == 1).all()) and bool((lp < 0).all())


# ---- 6. determinism
def test_two_identical_calls_are_bit_identical():
    dd, S = CASES["c1_s8"]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m, u = pos_model(d, P, run), _uniforms(d, S)
    a, b = _sampled(m, x, S, u, collect_states=True, trim=False), _sampled(m, x, S, u, collect_states=True, trim=False)
    for v, w in zip(a, b):
        assert np.array_equal(v, w)


def test_result_does_not_depend_on_what_the_workspace_held():
    """A call on the workspace a larger call left behind, overwritten with NaN, gives the bits of a call on a fresh one."""
    dd, S = CASES["group_plus_1"]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    u = _uniforms(d, S)
    fresh = _sampled(pos_model(d, P, run), x, S, u, collect_states=True, trim=False)
    m = pos_model(d, P, run)
    _sampled(m, x, 2 * S, _uniforms(d, 2 * S), trim=False)      # 2 S rollouts per video: a larger workspace
    ws = m._cws
    n_big = ws.numel()
    ws[:n_big // 4 * 4].view(torch.float32).fill_(float("nan"))
    again = _sampled(m, x, S, u, collect_states=True, trim=False)
    assert m._cws is ws and ws.numel() == n_big                  # the same, larger, poisoned workspace served the call
    for v, w in zip(fresh, again):
        assert np.array_equal(v, w)


# ---- 7. the generator path
def test_seeded_generator_is_reproducible_and_equals_explicit_uniforms():
    d = po.make_dims(**po.POS_CFG["tiny"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    S = 4
    g = torch.Generator(device="cuda")
    outs = []
    with torch.no_grad():
        for _ in range(2):
            g.manual_seed(1234)
            outs.append(m.sample_templates(*cuda_inputs(x), S, generator=g, collect_states=True, trim=False))
        g.manual_seed(1234)
        u = torch.rand(d.B, S, d.L, device="cuda", generator=g)
        outs.append(m.sample_templates(*cuda_inputs(x), S, uniforms=u, collect_states=True, trim=False))
        g.manual_seed(4321)
        other = m.sample_templates(*cuda_inputs(x), S, generator=g, trim=False)
    for o in outs[1:]:
        for v, w in zip(outs[0], o):
            assert torch.equal(v, w)
    assert not torch.equal(other[0], outs[0][0])                 # another seed draws other templates
    with pytest.raises(ValueError):
        m.sample_templates(*cuda_inputs(x), S, uniforms=torch.zeros(d.B, S, d.L, dtype=torch.float64))
    with pytest.raises(ValueError):
        m.sample_templates(*cuda_inputs(x), S, uniforms=torch.zeros(d.B, S + 1, d.L))
    with pytest.raises(ValueError):
        m.sample_templates(*cuda_inputs(x), S, temperature=0.0)
    with pytest.raises(ValueError):
        m.sample_templates(*cuda_inputs(x), 0)


# ---- 8. into the captioner
def test_caption_sampled_is_caption_with_templates_on_the_drawn_templates():
    from controllable_xgating_amd import caption_sampled, caption_with_templates
    dp = po.make_dims(**po.POS_CFG["mid"])
    dc = pg.make_dims(**CFG["mid"])
    assert (dp.K, dp.R, dp.F1, dp.F2) == (dc.K, dc.R, dc.F1, dc.F2)
    S = 4
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    pm = pos_model(dp, P, run)
    # the seeded captioner's greedy captions do not move with a POS vector of this size (|pos_feats| < 0.2), so its POS input is
    # weighed 16 times more: in the float64 oracle chain 15 of the 24 later slots then get another caption than slot 0
    Pc = pg.make_params(dc)
    Pc["lstmcore.lstm_1.a2h.weight"] = Pc["lstmcore.lstm_1.a2h.weight"] * np.float32(16.0)
    cap = make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    u = _uniforms(dp, S, seed=13)
    seq, slp, tm, score, first = caption_sampled(pm, cap, fr, fo, fm, S, temperature=1.3, uniforms=u, opt={"sample_max": 1})
    assert not seq.requires_grad and not slp.requires_grad and not score.requires_grad
    assert seq.shape[:2] == (dp.B, S) and slp.shape == seq.shape and tm.shape == (dp.B, S, dp.L) and score.shape == (dp.B, S)
    assert first.shape == (dp.B, S) and first.dtype == torch.bool
    seq_w, slp_w, score_w = caption_with_templates(pm, cap, fr, fo, fm, tm, {"sample_max": 1})
    assert torch.equal(seq, seq_w) and torch.equal(slp, slp_w) and torch.equal(score, score_w)
    with torch.no_grad():
        tm2, lp2, _, _, _ = pm.sample_templates(fr, fo, fm, S, temperature=1.3, uniforms=u, trim=False)
    assert torch.equal(tm, tm2) and torch.equal(score, lp2.sum(2))
    tn, sn = tm.cpu().numpy(), seq.cpu().numpy()
    host_first = np.array([[tuple(tn[b, s]) not in {tuple(r) for r in tn[b, :s]} for s in range(S)] for b in range(dp.B)])
    assert np.array_equal(first.cpu().numpy(), host_first) and host_first[:, 0].all()
    # the drawn templates matter: two different ones steer at least one video to different captions
    apart = [(b, s) for b in range(dp.B) for s in range(1, S)
             if not np.array_equal(tn[b, s], tn[b, 0]) and not np.array_equal(sn[b, s], sn[b, 0])]
    assert apart
