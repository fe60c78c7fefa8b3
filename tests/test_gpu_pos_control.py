"""Controlled POS generation on the MI355X: PosModel.sample_forced (include/xgate_pos_control.h) against the reference's own
outputs (tests/golden/pos_*.npz, fed their greedy tokens), against the greedy rollout bit for bit at one template per video,
against the float64 oracle (tests/pos_control_oracle.py in eager torch on the same GPU) at several templates per video over every
branch of the two new kernels, and control.caption_with_templates against the oracle chain into the captioner.

Bounds: those of tests/test_gpu_pos.py for this model -- states, pos_feats and masks 1e-4, log-probabilities 3e-4."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import pos_control_oracle as pco
from tests import pos_oracle as po
from tests.pos_control_oracle import cuda_inputs, golden_template, load_case, pos_model
from tests.util import CFG, assert_greedy_tokens_match, make_model

pytestmark = pytest.mark.gpu
F64 = torch.float64
ST_TOL, LP_TOL = 1e-4, 3e-4
GROUP = 4                                   # XGPC_TEMPLATE_GROUP (tests/test_pos_control_cpu.py pins the binding's copy to the header)

# name -> (dims, S): the smallest shapes at which each branch of pos_attn_group_kernel / pos_cell_head_rows_kernel<false> and of the
# launches around them can go wrong
SMALL = dict(E=18, C=5, L=6, F1=20, F2=12)
CASES = {
    "tiny_s3": (po.POS_CFG["tiny"], 3),                                             # 15 rows, nothing a multiple of 8
    "a_r_odd": (dict(B=3, K=5, R=22, A=38, **SMALL), 2),                            # A % 4 != 0 (scalar loads), R % 4 != 0
    "group_plus_1": (dict(po.POS_CFG["mid"], B=3), GROUP + 1),                      # a full group and a partial one of 1
    "k_past_prefetch": (dict(B=2, K=300, R=64, A=96, E=36, C=20, L=6, F1=48, F2=40), 3),   # ceil(K / nsplit) = 19 > 16 registers
    "serial_head": (dict(B=2, K=5, R=40, A=52, E=24, C=130, L=6, F1=20, F2=12), 3),  # C > 64
    "rows_297": (dict(po.POS_CFG["tiny"], B=9), 33),                                # > 256 rows: n_out, the products; 8 full groups + 1
    # 4 max(A, nsplit R) + A + 4 K floats of LDS pass 64 KiB: one template per workgroup, with float4 and with scalar loads
    "wide_a": (dict(B=2, K=5, R=24, A=3300, E=18, C=5, L=4, F1=20, F2=12), 3),
    "wide_a_odd": (dict(B=2, K=5, R=24, A=3301, E=18, C=5, L=4, F1=20, F2=12), 2),
    "c1_s8": (po.POS_CFG["c1"], 8),                                                 # the real layer sizes
}


def test_cases_reach_the_branches_they_name():
    from controllable_xgating_amd import _native_pos_control as npc
    assert npc.XGPC_TEMPLATE_GROUP == GROUP
    d, S = CASES["a_r_odd"]
    assert d["A"] % 4 and d["R"] % 4
    d, S = CASES["group_plus_1"]
    assert S % GROUP == 1 and S > GROUP
    d, S = CASES["k_past_prefetch"]
    nsplit = min(max(1024 // d["R"], 1), d["K"])                # xg_pos.hip: STEP_TPB / R, and VREG = 16
    assert -(-d["K"] // nsplit) > 16
    assert CASES["serial_head"][0]["C"] > 64
    d, S = CASES["rows_297"]
    assert d["B"] * S == 297 and S % GROUP
    d, S = CASES["tiny_s3"]
    assert d["B"] * S == 15 and S < GROUP

    def group_lds(d, G):                                         # xg_pos.hip: attn_group_lds
        nsplit = min(max(1024 // d["R"], 1), d["K"])
        r4 = lambda v: (v + 3) // 4 * 4
        return 4 * (r4(G * max(d["A"], nsplit * d["R"])) + r4(d["A"]) + G * d["K"])

    for name, (d, S) in CASES.items():
        wide = name.startswith("wide_a")
        assert (group_lds(d, GROUP) > 64 * 1024) == wide and group_lds(d, 1) <= 64 * 1024 and S > 1
    assert CASES["wide_a"][0]["A"] % 4 == 0 and CASES["wide_a_odd"][0]["A"] % 4


@functools.lru_cache(maxsize=None)
def _case(name):
    """(d, P, run, x, templates (B,S,L), lens, the float64 oracle's outputs as numpy) -- computed once, read-only."""
    dd, S = CASES[name]
    d = po.make_dims(**dd)
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=40 + len(name), ragged=True)
    tm, lens = pco.seeded_templates(d.B, S, d.L, d.C, seed=7 + len(name))
    Pt, rt = po.to_torch(P, F64, "cuda"), po.to_torch(run, F64, "cuda")
    fr, fo, fm = (torch.from_numpy(x[k]).to("cuda", F64) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    o = pco.sample_forced(Pt, rt, fr, fo, fm, tm, d.L)
    o = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()}
    return d, P, run, x, tm, lens, o


def _forced(m, x, tm, **kw):
    with torch.no_grad():
        out = m.sample_forced(*cuda_inputs(x), tm, **kw)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in out]


@pytest.mark.parametrize("name", list(po.GOLDEN_CASES))
def test_golden_tokens_reproduce_the_reference_goldens(name):
    d, P, run, x, g = load_case(name)
    tm, comparable = golden_template(d, g)
    lp, states, masks, pf = _forced(pos_model(d, P, run), x, torch.from_numpy(tm))
    n = int(g["n"])
    assert lp.shape == (d.B, 1, n) and states.shape == (d.B, 1, n + 1, d.R) and masks.shape == (d.B, 1, n + 1)
    cols = g["states"].shape[2]
    np.testing.assert_allclose(states[:, 0, :, :cols], g["states"], atol=ST_TOL)
    np.testing.assert_allclose(masks[:, 0], g["masks"], atol=ST_TOL)
    np.testing.assert_allclose(pf, g["pos_feat"], atol=ST_TOL)
    assert np.array_equal(pf, states[:, 0, n])
    np.testing.assert_allclose(lp[:, 0][comparable], g["seqLogprobs"][comparable], atol=LP_TOL)
    assert (lp[:, 0][~comparable] == 0).all()


@pytest.mark.parametrize("cfg", ["tiny", "c1"])
def test_one_template_per_video_is_bit_identical_to_greedy(cfg):
    """sample_forced fed the tokens PosModel.sample just chose walks the same states: same bits in states and masks."""
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    with torch.no_grad():
        seq, slp, st_g, mk_g = m.sample(*cuda_inputs(x), {"sample_max": 1})
        lp, st_f, mk_f, pf = m.sample_forced(*cuda_inputs(x), seq)                      # (B, n): one template per video
    n = seq.shape[1]
    assert n >= 1 and st_f.shape == (d.B, 1, n + 1, d.R)
    assert torch.equal(st_f[:, 0], st_g) and torch.equal(mk_f[:, 0], mk_g)
    assert torch.equal(pf, st_g[:, n])
    alive = torch.cat([torch.ones(d.B, 1, dtype=torch.bool, device="cuda"), (seq[:, :-1] > 0).cumprod(1).bool()], 1)
    np.testing.assert_allclose(lp[:, 0][alive].cpu().numpy(), slp[alive].cpu().numpy(), atol=LP_TOL)


@pytest.mark.parametrize("name", list(CASES))
def test_many_templates_vs_f64_oracle(name):
    d, P, run, x, tm, lens, o = _case(name)
    S = tm.shape[1]
    assert lens.reshape(-1)[0] == 0 and lens.max() == d.L and len(set(lens.reshape(-1).tolist())) > 2
    m = pos_model(d, P, run)
    lp, states, masks, pf = _forced(m, x, tm, trim=False)
    assert lp.shape == (d.B, S, d.L) and states.shape == (d.B, S, d.L + 1, d.R) and masks.shape == (d.B, S, d.L + 1)
    assert pf.shape == (d.B * S, d.R)
    for s in range(1, S):                                        # each slot got another template
        assert not np.array_equal(tm[:, s].numpy(), tm[:, 0].numpy())
    np.testing.assert_allclose(states, o["states"], atol=ST_TOL)
    assert np.array_equal(masks, o["masks"])
    np.testing.assert_allclose(pf, o["pos_feats"], atol=ST_TOL)
    np.testing.assert_allclose(lp, o["tag_logp"], atol=LP_TOL)
    after = np.arange(d.L)[None, None, :] > lens[:, :, None]
    assert (lp[after] == 0).all() and (lp[~after] < 0).all()
    np.testing.assert_allclose(lp.sum(2), o["tag_logp"].sum(2), atol=LP_TOL * d.L)
    assert np.array_equal(pf.reshape(d.B, S, d.R), states[:, :, d.L])
    # trimmed to the reference's n (here the full length: one template has no end tag), and without the states: same bits
    n = o["n"]
    assert n == d.L
    lp_t, st_t, mk_t, pf_t = _forced(m, x, tm)
    assert np.array_equal(lp_t, lp[:, :, :n]) and np.array_equal(st_t, states[:, :, :n + 1]) and np.array_equal(mk_t, masks[:, :, :n + 1])
    lp_n, st_n, mk_n, pf_n = _forced(m, x, tm, collect_states=False)
    assert st_n is None
    assert np.array_equal(pf_n, pf) and np.array_equal(pf_t, pf) and np.array_equal(lp_n, lp_t) and np.array_equal(mk_n, mk_t)


@pytest.mark.parametrize("name,keep", [("rows_297", 3), ("tiny_s3", 0)])
def test_n_is_the_longest_template(name, keep):
    """n_out = min(L, the most leading non-zero tags of any row): decided by one late row past the first 256, and 0 when every
    template is empty (pos_feats is then the state after BOS)."""
    d, P, run, x, tm, _, o = _case(name)
    S = tm.shape[1]
    t2 = torch.zeros_like(tm)
    t2[-1, -1, :keep] = tm[0, 1, :keep]                          # (slot (0,1) is the full-length template)
    lp, states, masks, pf = _forced(pos_model(d, P, run), x, t2)
    assert lp.shape == (d.B, S, keep) and states.shape == (d.B, S, keep + 1, d.R) and masks.shape == (d.B, S, keep + 1)
    assert (masks[:, :, 0] == 1).all() and masks[:, :, 1:].sum() == keep
    first = o["states"][:, :, 0]                                 # the step that feeds BOS does not depend on the template
    np.testing.assert_allclose(states[:, :, 0], first, atol=ST_TOL)
    rest = np.ones((d.B, S), bool)
    rest[-1, -1] = keep == 0
    assert np.array_equal(pf.reshape(d.B, S, d.R)[rest], states[:, :, 0][rest])


def test_tags_after_the_first_zero_change_no_bit():
    d, P, run, x, tm, lens, _ = _case("group_plus_1")
    clean = tm.clone()
    clean[torch.from_numpy(np.arange(d.L)[None, None, :] >= lens[:, :, None])] = 0
    assert not torch.equal(clean, tm)
    m = pos_model(d, P, run)
    a, b = _forced(m, x, tm, trim=False), _forced(m, x, clean, trim=False)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_two_identical_calls_are_bit_identical():
    d, P, run, x, tm, _, _ = _case("c1_s8")
    m = pos_model(d, P, run)
    a, b = _forced(m, x, tm, trim=False), _forced(m, x, tm, trim=False)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_result_does_not_depend_on_what_the_workspace_held():
    """A call on the workspace a larger call left behind, overwritten with NaN, gives the bits of a call on a fresh one."""
    d, P, run, x, tm, _, _ = _case("group_plus_1")
    fresh = _forced(pos_model(d, P, run), x, tm, trim=False)
    m = pos_model(d, P, run)
    big = torch.cat([tm, tm.flip(1)], 1)                         # 2 S templates per video: a larger workspace
    _forced(m, x, big, trim=False)
    ws = m._cws
    n_big = ws.numel()
    ws[:n_big // 4 * 4].view(torch.float32).fill_(float("nan"))
    again = _forced(m, x, tm, trim=False)
    assert m._cws is ws and ws.numel() == n_big                  # the same, larger, poisoned workspace served the call
    for u, v in zip(fresh, again):
        assert np.array_equal(u, v)


def test_two_templates_steer_one_video_apart():
    d, P, run, x, tm, _, o = _case("tiny_s3")
    lp, states, masks, pf = _forced(pos_model(d, P, run), x, tm, trim=False)
    pf = pf.reshape(d.B, -1, d.R)
    gap_o = np.abs(o["pos_feats"].reshape(d.B, -1, d.R)[:, 1] - o["pos_feats"].reshape(d.B, -1, d.R)[:, 2]).max(1)
    gap = np.abs(pf[:, 1] - pf[:, 2]).max(1)
    assert (gap_o > 100 * ST_TOL).all()                          # the oracle's own states differ by far more than the bound
    assert (gap > 50 * ST_TOL).all()


def test_caption_with_templates_matches_the_oracle_chain():
    """control.caption_with_templates at the POS and captioner `mid` shapes, 3 templates per video, against
    pos_control_oracle -> oracle.xgate_oracle.sample(mode='greedy') on the oracle's own pos_feats."""
    from controllable_xgating_amd import caption_with_templates
    dp = po.make_dims(**po.POS_CFG["mid"])
    dc = pg.make_dims(**CFG["mid"])
    assert (dp.K, dp.R, dp.F1, dp.F2) == (dc.K, dc.R, dc.F1, dc.F2)
    S = 3
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    tm, _ = pco.seeded_templates(dp.B, S, dp.L, dp.C, seed=11)
    Pc = pg.make_params(dc)
    cap = make_model(dc, Pc, train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, slp, score = caption_with_templates(pos_model(dp, P, run), cap, fr, fo, fm, tm, {"sample_max": 1})
    assert not seq.requires_grad and not slp.requires_grad and not score.requires_grad       # (it runs under no_grad itself)
    assert seq.shape[:2] == (dp.B, S) and slp.shape == seq.shape and score.shape == (dp.B, S)
    cfr, cfo, cfm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    o = pco.sample_forced(po.to_torch(P), po.to_torch(run), cfr, cfo, cfm, tm, dp.L)
    np.testing.assert_allclose(score.cpu().numpy(), o["tag_logp"].sum(2).numpy(), atol=LP_TOL * dp.L)
    with torch.no_grad():
        seq_o, _, lps = xo.sample(xo.to_torch_params(Pc), cfr.repeat_interleave(S, 0), cfo.repeat_interleave(S, 0),
                                  cfm.repeat_interleave(S, 0), o["pos_feats"], dc.L, mode="greedy", train=False,
                                  running=xo.new_running(dc), return_logp=True)
    assert_greedy_tokens_match(seq.reshape(dp.B * S, -1).cpu().numpy(), seq_o.numpy(), lps)
    # the templates matter to the captioner's input: rows of one video got different POS vectors
    pf = o["pos_feats"].reshape(dp.B, S, -1)
    assert float((pf[:, 0] - pf[:, 1]).abs().max()) > 1e-2


def test_train_mode_and_bad_templates_raise():
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = pos_model(d, po.make_params(d), po.make_running(d))
    x = po.make_inputs(d)
    ok = torch.zeros(d.B, d.L, dtype=torch.int64)
    with pytest.raises(ValueError):
        m.sample_forced(*cuda_inputs(x), torch.full((d.B, 2, d.L), d.C, dtype=torch.int64))       # out of range, on the CPU
    with pytest.raises(ValueError):
        m.sample_forced(*cuda_inputs(x), torch.zeros(d.B, d.L + 1, dtype=torch.int64).cuda())       # too long
    with pytest.raises(ValueError):
        m.sample_forced(*cuda_inputs(x), ok[:-1])                                                  # one video short
    m.train()
    with pytest.raises(NotImplementedError):
        m.sample_forced(*cuda_inputs(x), ok)
