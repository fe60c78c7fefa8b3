"""CPU checks of truncated (top-k / nucleus) caption sampling: the oracle's own properties on hand-made rows
(tests/cap_trunc_oracle.py implements docs/CAPTION_TRUNCATED.md), the untruncated oracle rollout against xo.sample, the C ABI of
include/xgate_truncate.h against its binding, every refusal without a GPU, and the CAP CONDITION of tests/test_gpu_cap_trunc.py:
for every (case, setting) the GPU file runs, the oracle in float32 differs from itself in float64 in at most 2 rows.  No compute
on a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import cap_trunc_oracle as co
from tests import util
from tests.util import ROOT

MAX_ROWS = 2                                                    # the cap test_gpu_cap_trunc.py allows per case


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- 1. the oracle's own properties
ROW = np.array([1.0, 3.0, 2.0, 3.0, -1.0, 2.0, 0.5, 2.0, -4.0])     # classes: 3 (x2), 2 (x3), 1, 0.5, -1, -4


def _kept(x, **kw):
    return set(np.flatnonzero(co.kept_set(np.asarray(x, float), **kw).mask).tolist())


def test_top_k_1_is_the_argmax_class():
    assert _kept(ROW, top_k=1) == {1, 3}
    assert _kept(ROW, top_k=1, top_p=0.3) == {1, 3} and _kept(ROW, top_k=1, temperature=0.5) == {1, 3}
    assert _kept([0.0, 5.0, 1.0], top_k=1) == {1}


def test_ties_at_the_kth_value_are_all_kept():
    assert _kept(ROW, top_k=2) == {1, 3}
    assert _kept(ROW, top_k=3) == _kept(ROW, top_k=4) == _kept(ROW, top_k=5) == {1, 3, 2, 5, 7}
    assert _kept(ROW, top_k=6) == {1, 3, 2, 5, 7, 0}


def test_both_off_keeps_everything():
    for kw in (dict(), dict(top_k=0, top_p=1.0), dict(top_k=len(ROW)), dict(top_k=len(ROW) + 5), dict(temperature=0.3)):
        k = co.kept_set(ROW, **kw)
        assert k.mask.all() and k.thr == ROW.min() and k.below == -np.inf


def test_the_nucleus_is_the_smallest_set_of_value_classes_reaching_the_mass():
    w = np.exp(ROW - ROW.max())
    Z = w.sum()
    classes = [v for v in sorted(set(ROW.tolist()), reverse=True)]
    cum = np.array([w[ROW >= v].sum() for v in classes])
    for p in (0.05, 0.3, 0.55, 0.56, 0.9, 0.95, 0.999, 0.9999999):
        k = co.kept_set(ROW, top_p=p)
        i = classes.index(k.thr)
        assert cum[i] >= p * Z and (i == 0 or cum[i - 1] < p * Z), p               # reaches it; one class fewer does not
        assert np.array_equal(k.mask, ROW >= k.thr) and k.mask[int(np.argmax(ROW))]
        assert k.mass_at == pytest.approx(cum[i]) and k.need == pytest.approx(p * Z)
    # a mass exactly on a class boundary keeps no further class: two equal words, p = 0.5 of a two-class row
    assert _kept([0.0, 0.0], top_p=0.5) == {0, 1}
    # the temperature enters the masses
    assert len(_kept(ROW, top_p=0.9, temperature=0.25)) < len(_kept(ROW, top_p=0.9, temperature=4.0))


def test_the_kept_set_does_not_depend_on_the_column_order():
    rng = np.random.RandomState(3)
    x = np.round(rng.randn(200) * 2, 1)                             # many ties
    for kw in (dict(top_k=17), dict(top_p=0.8), dict(top_k=40, top_p=0.6, temperature=0.7)):
        k = co.kept_set(x, **kw)
        for _ in range(3):
            perm = rng.permutation(x.size)
            kp = co.kept_set(x[perm], **kw)
            assert np.array_equal(kp.mask, k.mask[perm]) and kp.thr == k.thr and kp.mask.sum() == k.mask.sum()


def test_top_p_is_taken_inside_top_k():
    x = np.log(np.array([0.4, 0.3, 0.2, 0.1]))
    assert _kept(x, top_p=0.65) == {0, 1}
    assert _kept(x, top_k=2, top_p=0.65) == {0, 1}                  # 0.4 < 0.65 * 0.7 = 0.455
    assert _kept(x, top_k=2, top_p=0.55) == {0}                     # 0.4 >= 0.55 * 0.7 = 0.385, though 0.4 < 0.55 of the whole
    assert _kept(x, top_p=0.55) == {0, 1}
    k = co.kept_set(x, top_k=2, top_p=0.55)
    assert k.z_k == pytest.approx(0.7 / 0.4) and k.tau_k == x[1] and k.thr == x[0]


def test_signed_zeros_fall_in_one_class():
    x = np.array([-0.0, 0.0, -1.0, 0.0, -2.0])
    assert _kept(x, top_k=1) == {0, 1, 3} and _kept(x, top_k=2) == {0, 1, 3}
    assert _kept(np.array([0.0, -0.0, -1.0]), top_p=0.3) == {0, 1}
    assert _kept(np.array([1.0, -0.0, 0.0, -3.0]), top_k=2) == {0, 1, 2}


def test_the_draw_walks_the_kept_columns_in_column_order():
    x = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    # top_k = 2 keeps columns 1 (0.4) and 3 (0.3): the CDF is [0, 4/7, 4/7, 1]
    for u, tok in ((0.0, 1), (0.5, 1), (4 / 7 - 1e-9, 1), (4 / 7 + 1e-9, 3), (0.999999, 3)):
        t, lp, lq, kept, _, (lo, hi) = co.draw(x, u, top_k=2)
        assert (t, kept) == (tok, 2) and lo <= u < hi
        assert lp == pytest.approx(np.log([0.1, 0.4, 0.2, 0.3][tok])) and lq == pytest.approx(np.log([0, 4 / 7, 0, 3 / 7][tok]))
    t, lp, lq, kept, _, _ = co.draw(x, 0.7, top_k=1)
    assert (t, kept, lq) == (1, 1, 0.0)
    # tempered: logq follows the weights, logp does not
    t, lp, lq, kept, _, _ = co.draw(x, 0.9, temperature=0.5, top_k=2)
    assert t == 3 and lp == pytest.approx(np.log(0.3)) and lq == pytest.approx(np.log(0.09 / 0.25))


# ---- 2. the untruncated rollout is xo.sample
@pytest.mark.parametrize("name,temperature", [("tiny_s5", 1.0), ("mid_b3_s5", 0.7), ("odd_s2", 1.3)])
def test_untruncated_rollout_equals_the_oracle_sample(name, temperature):
    d, S, P, x, pos, u = co.inputs(name)
    r = co.rollout(co.context(name), u, temperature, 0, 1.0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        Pt = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in P.items()}
        rep = lambda k: torch.from_numpy(np.repeat(x[k], S, 0)).double()       # noqa: E731
        with torch.no_grad():
            seq, slp = xo.sample(Pt, rep("feats_rgb"), rep("feats_opfl"), rep("feat_mask"), torch.from_numpy(pos).double(), d.L,
                                 mode="sample", uniforms=u, temperature=temperature, train=False, running=xo.new_running(d))
    finally:
        torch.set_default_dtype(old)
    assert np.array_equal(r["seq"], seq.numpy())
    live = np.concatenate([np.ones((seq.shape[0], 1), bool), seq.numpy()[:, :-1] > 0], 1)
    assert np.abs(r["seq_logp"] - slp.numpy())[live].max() < 1e-10
    assert (r["kept"][live] == d.V).all() and (r["kept"][~live] == 0).all() and (r["seq_logq"][~live] == 0).all()
    if temperature == 1.0:
        assert np.abs(r["seq_logq"] - r["seq_logp"])[live].max() < 1e-10


# ---- 3. the cap condition of the GPU test
def test_the_peaked_case_has_a_nucleus_of_a_few_dozen_words():
    r = co.oracle("peaked", co.SETTINGS[0])
    flat = co.oracle("mid_b3_s5", co.SETTINGS[0])
    k, kf = r["kept"][r["kept"] > 0], flat["kept"][flat["kept"] > 0]
    print("p = 0.9 nucleus: peaked mean %.1f (min %d, max %d) of %d words, flat mean %.1f" % (k.mean(), k.min(), k.max(), 500, kf.mean()))
    assert 24 <= k.mean() <= 60 and kf.mean() > 300


@pytest.mark.parametrize("name,setting", co.PAIRS, ids=["%s-T%g-k%d-p%g" % ((n,) + s) for n, s in co.PAIRS])
def test_float32_oracle_differs_from_float64_in_at_most_two_rows(name, setting):
    a, b = co.oracle(name, setting), co.oracle(name, setting, torch.float32)
    rows = co.first_differences(a["seq"], b["seq"])
    krows = co.first_differences(a["kept"], b["kept"])
    print("%s %s: %d rows differ in seq, %d in kept, of %d" % (name, setting, len(rows), len(krows), a["seq"].shape[0]))
    assert len(rows) <= MAX_ROWS and len(krows) <= MAX_ROWS, (rows, krows)


# ---- 4. header, binding, refusals
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_truncate.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgtr_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgtr_rollout", "xgtr_version", "xgtr_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgtr_[a-z_0-9]+)\b", out))) == syms


def test_header_and_binding_agree(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_control as ncc
    from controllable_xgating_amd import _native_truncate as ntr
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "xgate_truncate.h"\nint main(void) {\n'
                   '  printf("%d %d %d\\n", XGTR_VERSION, XGCC_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    ver, cver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = ntr.lib()
    assert ver == ntr.XGTR_VERSION == L.xgtr_version() == 1 and cver == ncc.XGCC_VERSION and xver == nv.XG_VERSION
    # argument count and types of xgtr_rollout, from the declaration
    decl = re.search(r"int\s+xgtr_rollout\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    C = ctypes
    kinds = []
    for a in args:
        if "*" in a:
            kinds.append("ptr")
        else:
            kinds.append(a.rsplit(" ", 1)[0])
    want = {"ptr": None, "int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}
    got = L.xgtr_rollout.argtypes
    assert len(got) == len(args) == 18
    for a, k, g in zip(args, kinds, got):
        if k == "ptr":
            assert g is C.c_void_p or issubclass(g, C._Pointer), a
        else:
            assert g is want[k], (a, g)
    assert [k for k in kinds if k != "ptr"] == ["int32_t", "int32_t", "float", "float", "size_t"]
    assert L.xgtr_rollout.restype is C.c_int and L.xgtr_workspace_bytes.restype is C.c_size_t
    # no workspace of its own
    LC = ncc.lib()
    B = C.byref
    for cfg, S in (("tiny", 1), ("tiny", 5), ("mid", 3), ("c1", 8), ("odd", 2)):
        dm = _mk(pg.make_dims(**util.CFG[cfg]))
        assert L.xgtr_workspace_bytes(B(dm), S) == LC.xgcc_workspace_bytes(B(dm), S) > 0
    for S in (0, -1):
        assert L.xgtr_workspace_bytes(B(_mk(pg.make_dims(**util.CFG["mid"]))), S) == 0
    assert L.xgtr_workspace_bytes(None, 3) == 0


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_truncate as ntr
    L = ntr.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgtr_workspace_bytes(B(dims), 3)
    fake = 256
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

    def call(dm=dims, S=3, p=P, b=bn, x=None, r=None, k=5, tp=0.9, u=fake, temp=1.0, outs=None, ws=fake, nbytes=big):
        o = [fake] * 5 if outs is None else outs       # seq, seq_logp, seq_logq, kept, n_steps
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgtr_rollout(None, B(dm), S, None if p is None else B(p), None if b is None else B(b), None if x is False else B(x),
                              None if r is False else B(r), k, tp, u, temp, o[0], o[1], o[2], o[3], o[4], ws, nbytes)

    # every argument valid (pointers never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4 and call(S=4, nbytes=need) == -4
    assert call(k=0, tp=1.0, nbytes=8) == -4 and call(k=1 << 30, tp=1e-6, temp=0.1, nbytes=8) == -4
    assert call(outs=[fake, fake, None, None, fake], nbytes=8) == -4          # seq_logq and kept may be null
    # XG_EINVAL: the truncation's own
    assert call(k=-1) == -1 and call(k=-(1 << 31)) == -1
    for tp in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert call(tp=tp) == -1, tp
    assert call(u=None) == -1
    for temp in (0.0, -1.0, float("nan")):
        assert call(temp=temp) == -1, temp
    # ... and whatever the rollout over rows per video refuses
    assert call(S=0) == -1 and call(S=-2) == -1
    assert call(dm=_mk(d, B=0)) == -1 and call(dm=_mk(d, L=0)) == -1 and call(dm=_mk(d, B=1 << 10), S=(1 << 10) + 1) == -1
    assert call(r=run(train=1)) == -1 and call(r=run(save=1)) == -1
    assert call(r=run(gemm_mode=1)) == -1 and call(r=run(gemm_mode=3)) == -1
    assert call(b=None) == -1
    for i in range(4):
        st = [fake] * 4
        st[i] = None
        assert call(b=nv.XgBnState(*st)) == -1, i
    assert call(ws=fake + 16) == -1 and call(ws=None) == -1
    assert call(p=None) == -1 and call(x=False) == -1 and call(r=False) == -1
    for key in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"):
        assert call(x=batch(**{key: None})) == -1, key
    for i in (0, 1, 4):
        outs = [fake] * 5
        outs[i] = None
        assert call(outs=outs) == -1, i


def test_python_raises_without_a_gpu(built):
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import caption_truncated_with_templates
    assert "caption_truncated_with_templates" in pkg.__all__
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    with pytest.raises(NotImplementedError):                # train mode
        m.sample_truncated_per_video(*f, pos)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.sample_truncated_per_video(*f, pos, top_k=5, top_p=0.9)
    # bad truncation arguments: ValueError although the tensors are on the CPU (raised before the device gate)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")), dict(temperature=0.0),
               dict(temperature=-2.0), dict(temperature=float("inf")), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            m.sample_truncated_per_video(*f, pos, **kw)
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.sample_truncated_per_video(*f, bad)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.sample_truncated_per_video(*f, pos)
    m.precision = "fp32"

    # the wrapper: forced POS rollout, then the method, with the statistics behind the template score
    class Pos:
        def sample_forced(self, fr, fo, fm, templates, collect_states=False, trim=False):
            return torch.full((d.B, S, d.L), -0.5), None, None, torch.arange(d.B * S * d.R, dtype=torch.float32).reshape(d.B * S, d.R)

    class Cap:
        def sample_truncated_per_video(self, fr, fo, fm, pos_feats, **kw):
            self.got = (fr, fo, fm, pos_feats, kw)
            out = (torch.zeros(d.B, S, 4, dtype=torch.int64), torch.zeros(d.B, S, 4))
            return out + (torch.ones(d.B, S, 4), torch.ones(d.B, S, 4, dtype=torch.int32)) if kw["return_stats"] else out

    cap = Cap()
    u = torch.rand(d.L + 1, d.B * S)
    out = caption_truncated_with_templates(Pos(), cap, *f, None, top_k=7, top_p=0.8, temperature=0.9, uniforms=u)
    assert len(out) == 3 and out[2].shape == (d.B, S) and torch.all(out[2] == -0.5 * d.L)
    assert cap.got[0] is f[0] and cap.got[3].shape == (d.B, S, d.R)
    assert cap.got[4] == dict(top_k=7, top_p=0.8, temperature=0.9, uniforms=u, return_stats=False)
    out = caption_truncated_with_templates(Pos(), cap, *f, None, return_stats=True)
    assert len(out) == 5 and out[2].shape == (d.B, S) and out[3].dtype == torch.float32 and out[4].dtype == torch.int32
    assert cap.got[4] == dict(top_k=0, top_p=1.0, temperature=1.0, uniforms=None, return_stats=True)
    with pytest.raises(ValueError):
        caption_truncated_with_templates(Pos(), m, *f, None, top_p=0.0)
    with pytest.raises(NotImplementedError):                # CPU tensors, through the wrapper
        caption_truncated_with_templates(Pos(), m, *f, None, top_k=3)
