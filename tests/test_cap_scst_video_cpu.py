"""CPU checks of self-critical training on S rollouts per video (include/xgate_scst_video.h): the composed oracle
(tests/cap_scst_video_oracle.py) against xo.sample on the repeated batch, the advantage rules against a hand-computed table, the
preconditions of the GPU cases, the C ABI -- exports, version, workspace sizes, every refusal in the documented order without a GPU --,
the raises of SAModel.rollout_per_video and PerVideoRewardCriterion, and the Trainer path with the model calls stubbed.  No compute on
a GPU."""
import argparse
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import cap_scst_video_oracle as svo
from tests import util
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the oracle helper
@pytest.mark.parametrize("name", ["tiny_s5", "mid_b3_s5", "odd_s2", "one_s3"])
def test_composed_oracle_equals_sample_on_the_repeated_batch(name):
    """p = 0, train mode: the same tokens and log-probabilities as xo.sample on the batch with every video repeated S times."""
    dm, P, x, u = svo.repeated_inputs(name)
    s_c, lps_c = svo.case_draw(name)
    Pt, xi = xo.to_torch_params(P), xo.to_torch_inputs(x)
    with torch.no_grad():
        s_r, lp_r, lps_r = xo.sample(Pt, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], dm.L, mode="sample",
                                     uniforms=u, train=True, running=xo.new_running(dm), return_logp=True)
    assert np.array_equal(s_c, s_r.numpy())
    assert len(lps_c) == len(lps_r)
    for a, b in zip(lps_c, lps_r):
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=2e-6)


def test_replay_of_the_draw_gives_the_draw():
    name = "mid_b3_s5"
    d, S, P, xv, pos, u = svo.case_inputs(name)
    s, lps = svo.case_draw(name)
    Pt = xo.to_torch_params(P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    with torch.no_grad():
        so, lp = svo.composed_sample(Pt, t(xv["feats_rgb"]), t(xv["feats_opfl"]), t(xv["feat_mask"]), t(pos), S, d.L, "replay",
                                     forced=t(s), train=True, running=xo.new_running(d))
    assert np.array_equal(so.numpy(), s)
    for k in range(s.shape[1]):
        want = lps[k].numpy()[np.arange(s.shape[0]), s[:, k]]
        live = svo.reward_mask(s)[:, k]
        np.testing.assert_allclose(lp.numpy()[live, k], want[live], atol=1e-6)


def test_running_statistics_take_one_update_from_the_videos():
    """The composed oracle's BatchNorm update is that of the B videos: the unbiased factor over B K samples, not over B S K."""
    name = "mid_b3_s5"
    d, S, P, xv, pos, u = svo.case_inputs(name)
    dm, _, x, _ = svo.repeated_inputs(name)
    Pt = xo.to_torch_params(P)
    ra, rb = xo.new_running(d), xo.new_running(dm)
    xi, xr = xo.to_torch_inputs(xv), xo.to_torch_inputs(x)
    with torch.no_grad():
        xo.encoder_fwd(Pt, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], True, 0.0, 0, ra)
        xo.encoder_fwd(Pt, xr["feats_rgb"], xr["feats_opfl"], xr["feat_mask"], True, 0.0, 0, rb)
    n, nm = d.B * d.K, dm.B * d.K
    pre = xo.ENC + "visual_emb_rgb.1."
    np.testing.assert_allclose(ra[pre + "running_mean"].numpy(), rb[pre + "running_mean"].numpy(), atol=1e-7)
    va, vb = ra[pre + "running_var"].numpy(), rb[pre + "running_var"].numpy()
    np.testing.assert_allclose((va - 0.9) * (n - 1) / n, (vb - 0.9) * (nm - 1) / nm, rtol=1e-5, atol=1e-7)
    assert np.abs(va - vb).max() > 0


# ---- the criterion's reference
def test_advantage_rules_against_a_hand_computed_table():
    score = np.array([[1.0, 2.0, 6.0], [0.5, 0.5, 0.5]])
    np.testing.assert_array_equal(svo.advantages(score, None), score)
    np.testing.assert_allclose(svo.advantages(score, "mean_others"), [[1 - 4.0, 2 - 3.5, 6 - 1.5], [0.0, 0.0, 0.0]], rtol=0, atol=0)
    np.testing.assert_allclose(svo.advantages(score, "given", [2.0, -1.0]), [[-1.0, 0.0, 4.0], [1.5, 1.5, 1.5]], rtol=0, atol=0)
    with pytest.raises(AssertionError):
        svo.advantages(score[:, :1], "mean_others")
    # the criterion: two videos x two rows x three words; row (0, 1) ends at its first word, n cuts the last column
    seq = np.array([[[4, 2, 0], [0, 0, 0]], [[3, 0, 0], [5, 6, 7]]])
    slp = -np.arange(1.0, 13.0).reshape(2, 2, 3)
    adv = np.array([[1.0, -1.0], [2.0, 0.5]])
    m = svo.reward_mask(seq)
    assert m.astype(int).tolist() == [[[1, 1, 1], [1, 0, 0]], [[1, 1, 0], [1, 1, 1]]]
    loss, dslp = svo.criterion(slp, seq, adv)
    assert abs(loss - (1 * (1 + 2 + 3) - 1 * 4 + 2 * (7 + 8) + 0.5 * (10 + 11 + 12)) / 9) < 1e-12
    np.testing.assert_allclose(dslp[1, 1], [-0.5 / 9] * 3)
    loss2, dslp2 = svo.criterion(slp, seq, adv, n=2)
    assert abs(loss2 - (1 * (1 + 2) - 1 * 4 + 2 * (7 + 8) + 0.5 * (10 + 11)) / 7) < 1e-12 and (dslp2[..., 2] == 0).all()
    # against the oracle's RewardCriterion on the flattened rows
    ref = xo.reward_criterion(torch.from_numpy(slp.reshape(4, 3)), torch.from_numpy(seq.reshape(4, 3)),
                              torch.from_numpy(np.repeat(adv.reshape(4, 1), 3, 1)))
    assert abs(loss - ref.item()) < 1e-12


# ---- the cases
def test_cases_hold_what_they_name():
    for name, (cfg, over, S) in svo.CASES.items():
        d, S_, P, xv, pos, u = svo.case_inputs(name)
        M = d.B * S
        assert S_ == S and xv["feats_rgb"].shape == (d.B, d.K, d.F1) and pos.shape == (M, d.R) and u.shape == (d.L + 1, M)
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    c = {k: svo.cfg_of(k) for k in svo.CASES}
    assert (c["mid_b3_s5"]["B"], c["rows_132"]["B"], c["c1_s4"]["B"], c["c1_s4"]["L"], c["c5_s2"]["B"], c["mid_s1"]["B"]) == (3, 4, 2, 8, 2, 4)
    assert (c["c1_s4"]["R"], c["c1_s4"]["A"], c["c1_s4"]["K"], c["c1_s4"]["V"]) == (512, 1536, 26, 20000)
    d, S, _, xv, _, _ = svo.case_inputs("tiny_s5")
    assert (xv["feat_mask"] == 0).any()                                     # ragged feat_mask
    # rows_132: the named rows draw token 0 first and end there; other rows go on
    s, _ = svo.case_draw("rows_132")
    rows = list(svo.END_AT_FIRST_WORD["rows_132"])
    assert (s[rows] == 0).all() and (s[:, 0] > 0).sum() > 100 and s.shape[1] >= 2
    # every multi-row case keeps rows alive behind the first word and ends some row early or runs to L
    for name in svo.MULTI_ROW:
        s, _ = svo.case_draw(name)
        assert s.shape[1] >= 1 and (s[:, 0] > 0).any(), name


def test_cases_reach_the_branches_they_name():
    src = open(os.path.join(ROOT, "controllable_xgating_amd", "csrc", "xg_kernels.h")).read()
    assert int(re.search(r"XGK_ATTN_BWD_GROUP\s*=\s*(\d+)", src).group(1)) == svo.GROUP
    heads = open(os.path.join(ROOT, "controllable_xgating_amd", "csrc", "xg_heads.hip")).read()
    assert re.search(r"B >= 1 && B <= %d && R %% 32 == 0" % svo.SELECT_MAX_ROWS, heads)
    c = {k: svo.cfg_of(k) for k in svo.CASES}
    rows = {k: c[k]["B"] * v[2] for k, v in svo.CASES.items()}
    S = {k: v[2] for k, v in svo.CASES.items()}
    G = svo.GROUP
    # the step: LDS-staged (tiny), packed (mid, c1, c5), generic (odd: R % 8 != 0)
    assert not svo.packed(c["tiny_s5"]) and c["tiny_s5"]["R"] % 8 == 0
    assert svo.packed(c["mid_b3_s5"]) and svo.packed(c["c1_s4"]) and svo.packed(c["c5_s2"]) and svo.packed(c["rows_132"])
    assert c["odd_s2"]["R"] % 8 != 0 and not svo.packed(c["odd_s2"])
    # the choice: inside the step (mid_b3_s5, c1_s4, c5_s2, mid_s1), from the full logits (tiny: R; rows_132: rows; odd; one)
    for k in ("mid_b3_s5", "c1_s4", "c5_s2", "mid_s1"):
        assert svo.tile_statistics(c[k], rows[k]) and svo.choice_in_step(c[k], rows[k]), k
    for k in ("tiny_s5", "odd_s2", "one_s3", "rows_132"):
        assert not svo.tile_statistics(c[k], rows[k]), k
    assert rows["rows_132"] == 132 > svo.SELECT_MAX_ROWS and svo.tile_statistics(c["rows_132"], 128)
    # the s2-first launch order of the packed step from 65 rows on (core_step): rows_132 only
    assert rows["rows_132"] > 64 and all(rows[k] <= 64 for k in svo.CASES if k != "rows_132")
    # groups of the attention: a full group plus a partial one (S = 5), whole (S = 4), partial only (S = 2, 3, 1), many (S = 33)
    assert S["tiny_s5"] == G + 1 and S["mid_b3_s5"] == G + 1 and S["c1_s4"] == G and S["odd_s2"] < G and S["rows_132"] == 8 * G + 1
    # the per-step attention backward: group form but for odd
    assert all(svo.attn_bwd_group_form(c[k]) for k in svo.CASES if k != "odd_s2") and not svo.attn_bwd_group_form(c["odd_s2"])
    pieces = lambda d: -(-d["K"] // 8) * -(-d["R"] // 256)      # noqa: E731  (tests/test_cap_train_video_cpu.py)
    assert c["c5_s2"]["K"] > 32 and pieces(c["c5_s2"]) > 8 and c["c1_s4"]["K"] <= 32 and pieces(c["c1_s4"]) <= 8
    assert c["one_s3"]["K"] == 1 and c["one_s3"]["L"] == 1
    # the overlap split of heads_bwd needs T - 1 >= 4 steps: c1_s4 (8), mid (7), tiny (6), c5 (6); not odd (4 -> exactly 4), one (1)
    assert c["one_s3"]["L"] < 4 <= c["odd_s2"]["L"]


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_scst_video.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


SYMS = ["xgsv_reward_bwd", "xgsv_reward_fwd", "xgsv_rollout", "xgsv_rollout_bwd", "xgsv_version", "xgsv_workspace_bytes"]


def test_header_declarations_equal_library_exports(built):
    assert sorted(set(re.findall(r"\b(xgsv_[a-z_0-9]+)\s*\(", _header()))) == SYMS
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgsv_[a-z_0-9]+)\b", out))) == SYMS
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_scst_video.h":
            assert not re.search(r"xgsv_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h
    import __graft_entry__ as ge
    assert "xg_scst_video.hip" in ge.SOURCES


def test_version_through_gcc_and_xg_abi_unchanged(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_scst_video as nsv
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_scst_video.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(XgDims), sizeof(XgParams), sizeof(XgBnState), sizeof(XgBatch), '
                   'sizeof(XgRun), XGSV_VERSION, XG_VERSION, XGSV_BASE_NONE, XGSV_BASE_MEAN_OTHERS, XGSV_BASE_GIVEN);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[5] == nsv.XGSV_VERSION == nsv.lib().xgsv_version() == 1
    assert vals[6] == nv.XG_VERSION == 206
    assert tuple(vals[7:]) == (nsv.XGSV_BASE_NONE, nsv.XGSV_BASE_MEAN_OTHERS, nsv.XGSV_BASE_GIVEN) == (0, 1, 2)
    assert tuple(vals[:5]) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgParams, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_scst_video as nsv
    from controllable_xgating_amd import _native_train_video as ntv
    L = nsv.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    for S in (0, -1):
        assert L.xgsv_workspace_bytes(B(_mk(d)), S) == 0
    assert L.xgsv_workspace_bytes(None, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1), _mk(d, K=0)):
        assert L.xgsv_workspace_bytes(B(bad), 3) == 0
    assert L.xgsv_workspace_bytes(B(_mk(d, B=1 << 10)), (1 << 10) + 1) == 0    # beyond 2^20 rows
    # the real layer sizes at the length of a training rollout, B = 32 videos
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=32, L=30))
    T = c1.L + 1
    w = {S: L.xgsv_workspace_bytes(B(_mk(c1)), S) for S in (1, 2, 3, 4, 6, 8)}
    assert all(v > 0 for v in w.values())
    whole = nv.lib().xg_workspace_bytes_mode(B(_mk(c1, B=32 * 4)), 0)
    print("configs[2] layer sizes, L = 30, B = 32: xgsv_workspace_bytes S = 4 %d (%.1f MB), xg_workspace_bytes_mode(fp32) of the "
          "128-row batch %d (%.1f MB), xg_workspace_bytes %d" % (w[4], w[4] / 2 ** 20, whole, whole / 2 ** 20,
                                                                  nv.lib().xg_workspace_bytes(B(_mk(c1, B=128)))))
    assert w[4] < whole
    # no classifier tensors and no hoisted token side: below the teacher-forced per-video workspace of the same shape
    assert w[4] < ntv.lib().xgtv_workspace_bytes(B(_mk(c1)), 4)
    # linear in S between even S
    step = w[4] - w[2]
    assert step > 0 and w[6] - w[4] == step and w[8] - w[6] == step
    assert w[1] < w[2] < w[3] < w[4]
    # the per-row cost holds no K R or K A term: a further frame costs a row its alpha and de of the T steps only
    per_row = {}
    for K in (26, 58):
        dk = _mk(c1, K=K)
        per_row[K] = (L.xgsv_workspace_bytes(B(dk), 8) - L.xgsv_workspace_bytes(B(dk), 4)) / (4 * 32)
    per_frame = (per_row[58] - per_row[26]) / 32
    print("bytes per further row %.0f (K = 26), %.0f (K = 58): %.1f per frame and row (2 T floats = %d; one row of V alone %d)"
          % (per_row[26], per_row[58], per_frame, 8 * T, 4 * c1.R))
    assert per_frame == 8 * T
    assert per_frame < 4 * c1.R and per_frame < 4 * c1.A


def test_recorded_tables_are_untouched():
    for name, want in (("ws_sizes.json", "29f23468e4fd31f3f46c0e0c0f2c998587fc39ff8f7dceb32b871122a8b9f395"),
                       ("gemm_routes.json", "db9fb54b7f4694fb151a22acf40adfe4463cd2385b1dd3e410890155403d45c8")):
        got = hashlib.sha256(open(os.path.join(ROOT, "tests", "golden", name), "rb").read()).hexdigest()
        assert got == want, name


def test_bad_arguments_return_error_codes_in_the_documented_order_without_a_gpu(built):
    """The gate order of xgtv_xe_loss_fwd: bad dims (S among them) or a NULL workspace -1, a workspace that is too small -4 --
    whatever else is wrong with the call --, a misaligned workspace -1, and only then the entry point's own pointer and run tests
    -1.  Every pointer is a fake that is never dereferenced: nothing is enqueued."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_scst_video as nsv
    L = nsv.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgsv_workspace_bytes(B(dims), 3)
    fake = 0x7F0000000000
    P = nv.XgParams(*([fake] * len(nv.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def batch(**kw):
        v = dict(feats_rgb=fake, feats_opfl=fake, feat_mask=fake, pos_feats=fake)
        v.update(kw)
        return nv.XgBatch(**v)

    def run(**kw):
        r = nv.XgRun()
        r.bn_momentum, r.bn_eps, r.train = 0.1, 1e-5, 1
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def ref(o):
        return None if o is None or o is False else B(o)

    def fwd(dm=dims, S=3, p=P, b=bn, x=None, r=None, u=fake, temp=1.0, seq=fake, slp=fake, n=fake, ws=fake, nbytes=big, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgsv_rollout(None, ref(dm), S, ref(p), ref(b), ref(x), ref(r), u, temp, seq, slp, n, ws, nbytes)

    def bwd(dm=dims, S=3, p=P, g=P, x=None, r=None, dslp=fake, ws=fake, nbytes=big, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgsv_rollout_bwd(None, ref(dm), S, ref(p), ref(g), ref(x), ref(r), dslp, ws, nbytes)

    first = (dict(S=0), dict(S=-2), dict(dm=None), dict(dm=_mk(d, B=0)), dict(dm=_mk(d, L=0)), dict(dm=_mk(d, V=1)),
             dict(dm=_mk(d, B=1 << 10), S=(1 << 10) + 1), dict(ws=None))
    later = [dict(p=None), dict(x=False), dict(r=False), dict(r=run(gemm_mode=1)), dict(r=run(gemm_mode=3)), dict(ws=fake + 16)]
    later += [dict(x=batch(**{k: None})) for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats")]
    own_fwd = [dict(u=None), dict(seq=None), dict(slp=None), dict(n=None), dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")),
               dict(r=run(train=0), b=None), dict(r=run(train=0), b=nv.XgBnState(fake, None, fake, fake))]
    for call, own in ((fwd, own_fwd), (bwd, [dict(g=None), dict(dslp=None)])):
        mine = later + own
        for kw in first:                              # 1. -1, also with a workspace that is too small
            assert call(**kw) == -1 and call(**dict(kw, nbytes=8)) == -1, (call.__name__, kw)
        assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4            # 2. too small: -4, whatever else is wrong behind it
        assert call(S=4, nbytes=need) == -4                                    # the workspace of S = 3 does not serve S = 4
        for kw in mine:
            assert call(**dict(kw, nbytes=8)) == -4, (call.__name__, kw)
        for kw in mine:                               # 3. everything else: -1
            assert call(**kw) == -1, (call.__name__, kw)
            assert call(**dict(kw, nbytes=need)) == -1, (call.__name__, kw)

    # the criterion's entry points: nothing is enqueued for a refused call
    def rf(slp=fake, seq=fake, score=fake, base=None, mode=1, n=None, Bv=2, S=3, Lw=4, adv=fake, part=fake, out=fake):
        return L.xgsv_reward_fwd(None, slp, seq, score, base, mode, n, Bv, S, Lw, adv, part, out)

    for kw in (dict(slp=None), dict(seq=None), dict(score=None), dict(adv=None), dict(part=None), dict(out=None), dict(Bv=0), dict(S=0),
               dict(Lw=0), dict(Bv=1 << 10, S=(1 << 10) + 1), dict(Lw=(1 << 10) + 1), dict(mode=3), dict(mode=-1), dict(mode=1, S=1),
               dict(mode=2, base=None)):
        assert rf(**kw) == -1, kw

    def rb(seq=fake, adv=fake, Bv=2, S=3, Lw=4, sums=fake, dslp=fake):
        return L.xgsv_reward_bwd(None, seq, adv, None, Bv, S, Lw, sums, None, dslp)

    for kw in (dict(seq=None), dict(adv=None), dict(sums=None), dict(dslp=None), dict(Bv=0), dict(S=0), dict(Lw=0)):
        assert rb(**kw) == -1, kw


# ---- the Python surface
def test_rollout_per_video_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.rollout_per_video(*f, pos)
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.rollout_per_video(*f, bad)
    for bad in ((f[0][1:], f[1], f[2]), (f[0], f[1][:, 1:], f[2]), (f[0], f[1], f[2][:, 1:]), (f[0][:, :, 1:], f[1], f[2]),
                (f[0].reshape(d.B * d.K, -1), f[1], f[2])):
        with pytest.raises(ValueError):
            m.rollout_per_video(*bad, pos)
    for bad in (torch.rand(d.L, d.B * S), torch.rand(d.L + 1, d.B), torch.rand(d.L + 1, d.B, S), [0.5]):
        with pytest.raises(ValueError):
            m.rollout_per_video(*f, pos, uniforms=bad)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            m.rollout_per_video(*f, pos, temperature=bad)
    with pytest.raises(NotImplementedError):                # ... also with well-formed uniforms, and in eval mode
        m.rollout_per_video(*f, pos, uniforms=torch.rand(d.L + 1, d.B * S))
    m.eval()
    with pytest.raises(NotImplementedError):
        m.rollout_per_video(*f, pos)
    m.train()
    for prec in ("bf16", "bf16x3"):
        m.precision = prec
        with pytest.raises(NotImplementedError):
            m.rollout_per_video(*f, pos)


def test_per_video_reward_criterion_raises(built):
    from controllable_xgating_amd import PerVideoRewardCriterion
    crit = PerVideoRewardCriterion()
    assert crit.last_advantage is None
    B, S, L = 2, 3, 4
    slp, seq, score = torch.zeros(B, S, L), torch.zeros(B, S, L, dtype=torch.int64), torch.zeros(B, S)
    for args, kw in (((slp.reshape(B * S, L), seq, score), {}), ((slp, seq[:, :2], score), {}), ((slp, seq, score[:, :2]), {}),
                     ((slp, seq, score.reshape(-1)), {}), ((slp, seq, score), dict(baseline="greedy")),
                     ((slp, seq, score), dict(baseline=torch.zeros(B + 1))), ((slp, seq, score), dict(baseline=torch.zeros(B, S))),
                     ((slp[:, :1], seq[:, :1], score[:, :1]), dict(baseline="mean_others"))):
        with pytest.raises(ValueError):
            crit(*args, **kw)
    for base in ("mean_others", None, torch.zeros(B)):
        with pytest.raises(NotImplementedError):            # CPU tensors
            crit(slp, seq, score, baseline=base)


# ---- the Trainer path, the model calls stubbed
class _StubModel(torch.nn.Module):
    """What Trainer touches of SAModel, on the CPU: rollout_per_video returns fixed tokens and log-probs that depend on `w`."""

    def __init__(self, B, L):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.ss_prob, self.seq_length, self.calls = 0.0, L, []

    def rollout_per_video(self, f1, f2, fm, pos, temperature=1.0, uniforms=None, trim=False):
        B, S = pos.shape[:2]
        self.calls.append(("rollout_per_video", tuple(pos.shape)))
        seq = torch.arange(1, B * S * self.seq_length + 1).reshape(B, S, self.seq_length) % 7
        seq[:, :, 3:] = 0
        return seq, -self.w * torch.ones(B, S, self.seq_length), torch.tensor([3], dtype=torch.int32)

    def sample(self, f1, f2, fm, pos, opt={}):
        self.calls.append(("sample", tuple(pos.shape), opt.get("sample_max")))
        return torch.full((f1.shape[0], 2), 5, dtype=torch.int64), torch.zeros(f1.shape[0], 2)


class _StubCriterion:
    def __init__(self):
        self.calls, self.last_advantage = [], None

    def __call__(self, slp, seq, score, n=None, baseline="mean_others"):
        self.calls.append((tuple(slp.shape), tuple(score.shape), baseline if isinstance(baseline, str) else tuple(baseline.shape), n))
        base = None if isinstance(baseline, str) else baseline.numpy()
        adv = svo.advantages(score.numpy(), "mean_others" if base is None else "given", base)
        self.last_advantage = torch.from_numpy(adv)
        m = torch.from_numpy(svo.reward_mask(seq.numpy(), int(n)))
        return (-slp * self.last_advantage.unsqueeze(2).float() * m).sum() / m.sum()


def _stub_trainer(model, scorer, **kw):
    from controllable_xgating_amd.driver import Trainer
    opt = argparse.Namespace(learning_rate=1e-2, weight_decay=0.0, grad_clip=0.1, overlap_update=False, learning_rate_decay_start=-1,
                             scheduled_sampling_start=-1, self_critical_after=0, **kw)
    tr = Trainer.__new__(Trainer)                        # (no ClipAdam: it needs the GPU)
    tr.model, tr.opt, tr.scorer, tr.grad_sync, tr.iteration, tr.fused = model, opt, scorer, _StubArm(), 1, True
    tr.optimizer = _StubOptimizer(model)
    tr.start_epoch(0)
    assert tr.sc_flag
    tr.rl_crit_video = _StubCriterion()
    return tr


class _StubArm:
    def __init__(self):
        self.armed = 0

    def arm(self):
        self.armed += 1


class _StubOptimizer(_StubArm):
    def __init__(self, model):
        super().__init__()
        self.model, self.steps = model, 0

    def zero_grad(self):
        self.model.w.grad = None

    def set_lr(self, lr):
        self.lr = lr

    def step(self):
        assert self.model.w.grad is not None and self.armed == self.steps + 1       # armed before the backward, once per iteration
        self.steps += 1


def test_trainer_takes_the_per_video_path_with_the_model_calls_stubbed():
    B, S, L, R = 2, 3, 5, 4
    seen = []

    def scorer(rows, greedy):
        seen.append((rows.shape, None if greedy is None else greedy.shape))
        n = rows.shape[0] + (0 if greedy is None else greedy.shape[0])
        return np.arange(n, dtype=np.float64) / 10

    batch = dict(feat1=torch.zeros(B, 2, 3), feat2=torch.zeros(B, 2, 3), feat_mask=torch.ones(B, 2), pos_feat=torch.rand(B, R))
    # (B,R) pos_feat expanded to S rows; "mean_others" is the default and runs no greedy rollout
    m = _StubModel(B, L)
    tr = _stub_trainer(m, scorer, scst_rows_per_video=S)
    info = tr.train_batch(batch)
    assert m.calls == [("rollout_per_video", (B, S, R))] and seen == [((B * S, 3), None)]
    assert tr.rl_crit_video.calls[0][:3] == ((B, S, L), (B, S), "mean_others")
    np.testing.assert_allclose(tr.last_advantage.numpy(), svo.advantages(np.arange(6).reshape(2, 3) / 10), atol=1e-6)
    assert abs(info["avg_reward"] - 0.25) < 1e-6 and torch.isfinite(info["loss"]) and m.w.grad is not None
    assert tr.optimizer.steps == 1 and tr.grad_sync.armed == 1 and tr.iteration == 2
    # a (B,S,R) pos_feat takes the path without the option
    m = _StubModel(B, L)
    tr = _stub_trainer(m, scorer)
    pos3 = torch.rand(B, S, R)
    tr.train_batch(dict(batch, pos_feat=pos3))
    assert m.calls == [("rollout_per_video", (B, S, R))]
    # "greedy": sample(sample_max 1) on the B videos, base = score(greedy), scorer(rows, greedy) -> M + B scores
    seen.clear()
    m = _StubModel(B, L)
    tr = _stub_trainer(m, scorer, scst_rows_per_video=S, scst_baseline="greedy")
    info = tr.train_batch(batch)
    assert m.calls == [("sample", (B, R), 1), ("rollout_per_video", (B, S, R))] and seen == [((B * S, 3), (B, 2))]
    assert tr.rl_crit_video.calls[0][2] == (B,)
    np.testing.assert_allclose(tr.last_advantage.numpy(), np.arange(6).reshape(2, 3) / 10 - np.array([[0.6], [0.7]]), atol=1e-6)
    assert abs(info["avg_reward"] - (0.25 - 0.65)) < 1e-6
    with pytest.raises(NotImplementedError):
        tr.train_batch(dict(batch, pos_feat=pos3))
    # S = 1 without a three-dimensional pos_feat stays on the existing path (the stub has no sample_pair: it would raise)
    m = _StubModel(B, L)
    tr = _stub_trainer(m, scorer, scst_rows_per_video=1, scst_rollout_mode="sequential")
    with pytest.raises(Exception):
        tr.train_batch(batch)
    assert m.calls and m.calls[0][0] == "sample"


def test_scst_rollouts_per_video_raises():
    from controllable_xgating_amd.driver import scst_rollouts_per_video
    m = _StubModel(2, 5)
    f = (torch.zeros(2, 2, 3), torch.zeros(2, 2, 3), torch.ones(2, 2))
    with pytest.raises(ValueError):
        scst_rollouts_per_video(m, *f, torch.zeros(2, 4))                          # (B,R) without rows_per_video
    with pytest.raises(ValueError):
        scst_rollouts_per_video(m, *f, torch.zeros(2, 3, 4), rows_per_video=2)      # S against the option
    with pytest.raises(ValueError):
        scst_rollouts_per_video(m, *f, torch.zeros(2, 3, 4), baseline="mean")
    with pytest.raises(NotImplementedError):
        scst_rollouts_per_video(m, *f, torch.zeros(2, 3, 4), baseline="greedy")
    gen, slp, n, greedy = scst_rollouts_per_video(m, *f, torch.zeros(2, 4), rows_per_video=3)
    assert gen.shape == (2, 3, 5) and greedy is None and m.calls == [("rollout_per_video", (2, 3, 4))]
