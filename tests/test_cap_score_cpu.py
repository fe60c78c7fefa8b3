"""CPU checks of scoring given captions (include/xgate_score.h): the test oracle against a second route of the oracle, the
preconditions of the GPU cases (tests/test_gpu_cap_score.py), the C ABI -- exports, version, workspace sizes, every refusal in the
documented order without a GPU -- control.template_recovery, and the raises of SAModel.score_captions_per_video.  No compute on a
GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_score_oracle as cso
from tests import util
from tests.cap_score_oracle import LP_TOL
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the oracle helper
@pytest.mark.parametrize("name", ["tiny_q3", "mid_b3_q5", "odd_q2"])
def test_replay_helper_equals_the_teacher_forced_route_exactly(name):
    d, Q, P, x, pos, tokens = cso.case_inputs(name)
    a = cso.case_reference(name)
    b = cso.score_rows_xe(P, x, pos, tokens, Q)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    tok_logp, score, count = a
    cnt = cso.counted_columns(tokens)
    assert count.dtype == np.int32 and np.array_equal(count, cnt.sum(1)) and count.min() >= 1 and count.max() <= d.L
    assert (tok_logp[~cnt] == 0).all() and (tok_logp[cnt] < 0).all() and np.allclose(score, tok_logp.sum(1))


def test_counted_columns_by_hand():
    t = np.array([[0, 0, 0], [5, 0, 3], [5, 3, 0], [5, 3, 2], [0, 4, 4]])
    assert cso.counted_columns(t).astype(int).tolist() == [[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 1, 1], [1, 0, 0]]


# ---- preconditions of the GPU cases
def test_every_case_holds_the_edge_captions():
    for name, (dd, Q, _) in cso.cases().items():
        d, _, _, _, _, tok = cso.case_inputs(name)
        M, L, V = d.B * Q, d.L, d.V
        assert tok.shape == (M, L) and tok.min() >= 0 and tok.max() < V, name
        assert (tok[0] == 0).all(), name                                        # an empty caption
        assert any((r > 0).all() for r in tok), name                            # a caption without EOS
        assert any(r[L - 1] == 0 and (r[:L - 1] > 0).all() for r in tok), name  # an EOS in the last column (L = 1: the empty one)
        cnt = cso.counted_columns(tok)
        targets = set(tok[cnt].tolist())
        last = ((V - 1) // cso.TILE) * cso.TILE
        assert {0, 1, V - 1} <= targets and any(t >= last for t in targets), name
        if L >= 3:
            assert max(1, last) in targets, name                                # the first column of the last vocabulary tile


@pytest.mark.parametrize("name", list(cso.cases()))
def test_rows_of_one_video_are_well_apart(name):
    """Any two rows of one video differ by at least 100 LP_TOL in some column counted for both: a row misplaced within its video
    cannot pass the GPU comparison."""
    d, Q, _, _, _, tokens = cso.case_inputs(name)
    lp = cso.case_reference(name)[0]
    cnt = cso.counted_columns(tokens)
    worst = np.inf
    for b in range(d.B):
        r = slice(b * Q, (b + 1) * Q)
        diff = np.abs(lp[r][:, None, :] - lp[r][None, :, :])
        both = cnt[r][:, None, :] & cnt[r][None, :, :]
        mx = np.where(both, diff, 0.0).max(2)
        mx[np.arange(Q), np.arange(Q)] = np.inf
        worst = min(worst, mx.min())
    print("%s: two rows of one video differ by at least %.4f" % (name, worst))
    assert worst >= 100 * LP_TOL


def test_hot_case_is_past_fp32_exp_overflow_and_its_float32_oracle_holds():
    d, Q, P, x, pos, tokens = cso.case_inputs("hot")
    mx = []
    cso.score_rows_xe(P, x, pos, tokens, Q, raw_logit_max=mx)
    dev = np.abs(cso.case_reference("hot", torch.float32)[0] - cso.case_reference("hot")[0]).max()
    print("hot: max raw logit %.1f, float32 oracle deviates by %.2e" % (mx[0], dev))
    assert mx[0] > 88.7
    assert dev <= LP_TOL / 4


def test_cases_reach_the_shapes_they_name():
    c = {k: v[0] for k, v in cso.cases().items()}
    q = {k: v[1] for k, v in cso.cases().items()}
    fast = lambda d: d["R"] % 32 == 0 and d["V"] >= cso.TILE      # noqa: E731  (xg_score.hip: score_fast, operands aligned)
    assert fast(c["mid_b3_q5"]) and c["mid_b3_q5"]["V"] % cso.TILE and c["mid_b3_q5"]["L"] > 2 * cso.CHUNK
    assert not fast(c["odd_q2"]) and not fast(c["one_q3"]) and not fast(c["tiny_q3"]) and not fast(c["rows_297"])
    assert c["one_q3"]["L"] == 1 and c["one_q3"]["K"] == 1 and c["one_q3"]["V"] == 5
    for name in ("rows_297", "rows_297_r32"):
        assert c[name]["B"] * q[name] == 297
    assert fast(c["rows_297_r32"]) and 2 * cso.ROW_TILE < 297 < 3 * cso.ROW_TILE                    # three row tiles, the last partial
    assert fast(c["c1_q8"]) and c["c1_q8"]["V"] == 20000 and c["c1_q8"]["L"] % cso.CHUNK            # a partial last chunk
    assert fast(c["mid_v4100"]) and c["mid_v4100"]["V"] % cso.TILE == 4
    assert fast(c["hot"]) and cso.cases()["hot"][2] == 512.0


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_score.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgsc_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgsc_score_captions", "xgsc_version", "xgsc_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgsc_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_score.h":
            assert not re.search(r"xgsc_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_score as nsc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_score.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGSC_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ver == nsc.XGSC_VERSION == nsc.lib().xgsc_version() == 1
    assert xver == nv.XG_VERSION == 206
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_score as nsc
    L = nsc.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    sizes = [L.xgsc_workspace_bytes(B(_mk(d)), Q) for Q in range(1, 10)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))      # grows with Q
    for Q in (0, -1):
        assert L.xgsc_workspace_bytes(B(_mk(d)), Q) == 0
    assert L.xgsc_workspace_bytes(None, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1), _mk(d, K=0)):
        assert L.xgsc_workspace_bytes(B(bad), 3) == 0
    assert L.xgsc_workspace_bytes(B(_mk(d, B=1 << 10)), 1 << 10) > 0           # 2^20 rows
    assert L.xgsc_workspace_bytes(B(_mk(d, B=1 << 10)), (1 << 10) + 1) == 0    # ... and beyond
    assert L.xgsc_workspace_bytes(B(_mk(d, B=1 << 20)), 2) == 0
    # the real layer sizes: a further row costs less than ONE row of logits -- the workspace holds no (rows, V) tensor
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=64))
    w64, w32 = L.xgsc_workspace_bytes(B(_mk(c1)), 64), L.xgsc_workspace_bytes(B(_mk(c1)), 32)
    per_row = (w64 - w32) / (64 * 32)
    replay = nv.lib().xg_workspace_bytes_mode(B(_mk(c1, B=64 * 64)), 0)
    print("configs[1] dims, B = 64: xgsc_workspace_bytes Q = 64 %d (%.1f MB), Q = 32 %d; %.0f bytes per further row (4 V = %d); "
          "xg_workspace_bytes_mode of the 4096-row replay %d (%.1f MB)" % (w64, w64 / 2 ** 20, w32, per_row, 4 * c1.V, replay, replay / 2 ** 20))
    assert 0 < per_row < 4 * c1.V
    assert w64 < replay


def test_bad_arguments_return_error_codes_in_the_documented_order_without_a_gpu(built):
    """As tests/test_abi_cpu.py documents for every workspace-taking export: bad dims (Q among them) or a NULL workspace -1, a
    workspace that is too small -4 -- whatever else is wrong with the call --, a misaligned workspace -1, and only then the entry
    point's own pointer and run tests -1.  Every pointer is a fake that is never dereferenced: nothing is enqueued."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_score as nsc
    L = nsc.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgsc_workspace_bytes(B(dims), 3)
    fake = 0x7F0000000000
    P = nv.XgParams(*([fake] * len(nv.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def batch(**kw):
        v = dict(feats_rgb=fake, feats_opfl=fake, feat_mask=fake, pos_feats=fake, seq=None, seq_mask=None)
        v.update(kw)
        return nv.XgBatch(**v)

    def run(**kw):
        r = nv.XgRun()
        r.bn_momentum, r.bn_eps = 0.1, 1e-5
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def call(dm=dims, Q=3, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 4 if outs is None else outs       # tokens, tok_logp, score, count
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgsc_score_captions(None, None if dm is None else B(dm), Q, None if p is None else B(p), None if b is None else B(b),
                                     None if x is False else B(x), None if r is False else B(r), o[0], o[1], o[2], o[3], ws, nbytes)

    later = [dict(p=None), dict(x=False), dict(r=False), dict(b=None), dict(r=run(train=1)), dict(r=run(save=1)), dict(r=run(gemm_mode=1)),
             dict(r=run(gemm_mode=3)), dict(ws=fake + 16)]
    later += [dict(x=batch(**{k: None})) for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats")]
    for i in range(4):
        st = [fake] * 4
        st[i] = None
        later += [dict(b=nv.XgBnState(*st)), dict(outs=st)]
    # 1. bad dims, Q, too many rows, a NULL workspace: -1, also with a workspace that is too small
    for kw in (dict(Q=0), dict(Q=-2), dict(dm=None), dict(dm=_mk(d, B=0)), dict(dm=_mk(d, L=0)), dict(dm=_mk(d, V=1)),
               dict(dm=_mk(d, B=1 << 10), Q=(1 << 10) + 1), dict(ws=None)):
        assert call(**kw) == -1 and call(nbytes=8, **kw) == -1, kw
    # 2. too small: -4, whatever else is wrong behind it
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(Q=4, nbytes=need) == -4                                       # the workspace of Q = 3 does not serve Q = 4
    for kw in later:
        assert call(nbytes=8, **kw) == -4, kw
    # 3. everything else: -1
    for kw in later:
        assert call(**kw) == -1, kw
        assert call(nbytes=need, **kw) == -1, kw


# ---- control.template_recovery
def test_template_recovery_on_a_hand_made_matrix():
    from controllable_xgating_amd import template_recovery
    # score[b, s, n]: caption n under template s
    s = torch.tensor([[[-1.0, -5.0, -2.0],          # caption 0: best under its own template 0
                       [-2.0, -4.0, -2.0],          # caption 1: -4 under its own, -3 under template 2 -- not recovered
                       [-3.0, -3.0, -1.0]],         # caption 2: best under its own template 2
                      [[-1.0, -1.0, -9.0],          # captions 0 and 1 tie between templates 0 and 1: no template BEATS their own
                       [-1.0, -1.0, -9.0],
                       [-7.0, -7.0, -9.0]]])        # caption 2: the same under every template
    got = template_recovery(s)
    assert got.dtype == torch.bool and got.shape == (2, 3)
    assert got.tolist() == [[True, False, True], [True, True, True]]
    assert template_recovery(s.numpy()).tolist() == got.tolist()
    one = template_recovery(torch.zeros(4, 1, 1))
    assert one.shape == (4, 1) and bool(one.all())
    for bad in (torch.zeros(2, 3), torch.zeros(2, 3, 4), torch.zeros(2, 3, 3, 1)):
        with pytest.raises(ValueError):
            template_recovery(bad)


# ---- the Python surface
def test_score_captions_per_video_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    cap = torch.zeros(d.B, S, d.L, dtype=torch.int64)
    with pytest.raises(NotImplementedError):                # train mode
        m.score_captions_per_video(*f, pos, cap)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.score_captions_per_video(*f, pos, cap)
    with pytest.raises(NotImplementedError):
        m.score_captions_per_video(*f, pos, cap[:, :2], cross=True)
    bad_caps = (cap.float(), cap.bool(), cap[:, 0], cap[1:], cap[:, :0], cap.unsqueeze(0), torch.zeros(d.B, S, d.L + 1, dtype=torch.int64),
                cap[:, :2], torch.zeros(d.B, S + 1, d.L, dtype=torch.int32), cap.tolist())
    for bad in bad_caps:
        with pytest.raises(ValueError):
            m.score_captions_per_video(*f, pos, bad)
    for bad in (cap.float(), cap[1:], torch.zeros(d.B, 2, d.L + 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            m.score_captions_per_video(*f, pos, bad, cross=True)
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.score_captions_per_video(*f, bad, cap, cross=True)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.score_captions_per_video(*f, pos, cap)


def test_package_exports():
    import controllable_xgating_amd as pkg
    assert "score_captions_with_templates" in pkg.__all__ and "template_recovery" in pkg.__all__
    assert hasattr(pkg.SAModel, "score_captions_per_video")
