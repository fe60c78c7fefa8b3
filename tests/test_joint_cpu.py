"""CPU checks of joint training (docs/JOINT_TRAINING.md): the composed float64 oracle of tests/joint_oracle.py against central finite
differences, and the C ABI of include/xgate_joint.h and include/xgate_pos_joint.h (exports, versions, error codes without a GPU).
No compute on a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import joint_oracle as jo
from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the oracle
LAM = 0.5
# a handful of elements of each model's parameters: on the path the new gradient takes (the captioner's POS gate and first cell; the
# generator's recurrent weights, attention and initial state) and three that only the generator's own loss reaches.  No encoder
# parameter of either model: both init_hidden's detach the mean of V (SAModel.py:58-65, pos_src/SAModel.py:54-60), so the gradient
# the models train on is, for the encoders, not the derivative a finite difference measures.
CAP_ELEMS = (("lstmcore.gate.gate.0.weight", 7), ("lstmcore.lstm_1.a2h.weight", 101), ("lstmcore.lstm_2.h2h.weight", 55),
             ("logit.weight", 12), ("embed.weight", 3 * 18 + 4), ("img_embed_h_1.weight", 9))
POS_ELEMS = (("lstmcore.lstmcell.h2h.weight", 77), ("lstmcore.lstmcell.a2h.weight", 301), ("lstmcore.h2a.weight", 40),
             ("lstmcore.v2a.weight", 11), ("img_embed_h_1.weight", 5), ("img_embed_c_1.bias", 13),
             ("embed.weight", 2 * 18 + 1), ("logit.weight", 30), ("logit.bias", 2))


def _loss_at(which, name, idx, delta, lam, detach=False):
    dc, dp, Pc, Pp, run, x = jo.joint_case()
    dt = torch.float64
    Pc = {k: torch.from_numpy(np.asarray(v, np.float64).copy()) for k, v in Pc.items()}
    Pp = pto.params(Pp, dt, requires_grad=False)
    (Pc if which == "cap" else Pp)[name].view(-1)[idx] += delta
    with torch.no_grad():
        return jo.joint_loss(Pc, Pp, pto.running(run, dt), x, dc, lam, detach=detach)[0].item()


@pytest.mark.parametrize("lam,detach", [(LAM, False), (0.0, False)])
def test_composed_float64_gradient_against_central_differences(lam, detach):
    """(A detached pos_feats changes the gradient and not the function a finite difference sees: the test below covers it.)"""
    dc, dp, Pc, Pp, run, x = jo.joint_case()
    _, _, _, gc, gp = jo.joint_grads(Pc, Pp, run, x, dc, lam, detach=detach)
    h = 1e-6
    for which, elems, g in (("cap", CAP_ELEMS, gc), ("pos", POS_ELEMS, gp)):
        for name, idx in elems:
            fd = (_loss_at(which, name, idx, h, lam, detach) - _loss_at(which, name, idx, -h, lam, detach)) / (2 * h)
            an = float(g[name].reshape(-1)[idx])
            # float64 central differences at h = 1e-6: truncation ~ h^2 f''', round-off ~ 1e-16 |L| / h = 6e-10
            assert abs(fd - an) <= 1e-7 + 1e-5 * abs(an), (which, name, idx, fd, an)


def test_the_path_through_pos_feats_is_what_the_composition_adds():
    """lambda = 0: the generator's head gets exactly nothing and its recurrent weights something; detached: the generator's gradient
    is lambda times its own loss's and the captioner's is that of its loss on the constant vector."""
    dc, dp, Pc, Pp, run, x = jo.joint_case()
    _, _, _, _, g0 = jo.joint_grads(Pc, Pp, run, x, dc, 0.0)
    assert np.abs(g0["logit.weight"]).max() == 0.0 and np.abs(g0["logit.bias"]).max() == 0.0
    assert np.abs(g0["lstmcore.lstmcell.h2h.weight"]).max() > 1e-4 and np.abs(g0["two_fc_encoder.lstmcell_rgb.weight_hh"]).max() > 1e-6
    _, _, _, gc_l, gp_l = jo.joint_grads(Pc, Pp, run, x, dc, LAM)
    _, _, _, gc_d, gp_d = jo.joint_grads(Pc, Pp, run, x, dc, LAM, detach=True)
    _, _, _, _, gp_1 = jo.joint_grads(Pc, Pp, run, x, dc, 1.0, detach=True)
    for n in gp_d:
        np.testing.assert_allclose(gp_d[n], LAM * gp_1[n], rtol=1e-12, atol=1e-15)
    for n in gc_d:                                   # the captioner's own gradient does not depend on whether the path is cut
        np.testing.assert_allclose(gc_d[n], gc_l[n], rtol=1e-12, atol=1e-15)
    assert any(np.abs(gp_l[n] - gp_d[n]).max() > 1e-5 for n in gp_l)


def test_pos_forward_is_forward_train_with_the_state_kept():
    for name in ("tiny", "tfzero", "drop"):
        cfg, kw, p, seed = pto.TRAIN_CASES[name]
        d = po.make_dims(**po.POS_CFG[cfg])
        P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, **kw)
        r = jo.pos_reference(d, P, run, x, p, seed)
        loss, grads, _, _, out = pto.loss_and_grads(d, P, run, x, p, seed, dtype=torch.float64)
        assert r["logp"].shape == out.shape and np.abs(r["logp"] - out).max() < 1e-12 and abs(r["loss"] - loss) < 1e-12
        for n, g in grads.items():
            np.testing.assert_allclose(r["grads"][n], g, rtol=1e-10, atol=1e-14, err_msg=n)
        assert r["state"].shape == (d.B, d.R)
    assert r["logp"].shape[1] == d.L + 1
    cfg, kw, p, seed = pto.TRAIN_CASES["tfzero"]
    d = po.make_dims(**po.POS_CFG[cfg])
    assert jo.pos_reference(d, po.make_params(d), po.make_running(d), po.make_inputs(d, **kw))["logp"].shape[1] < d.L + 1


# ---- the C ABI
def _decl(header, prefix):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % prefix, txt)))


def test_header_declarations_equal_library_exports(built):
    want = {"xgj": ["xgj_caption_dpos", "xgj_last_kernel_width", "xgj_version"],
            "xgpj": ["xgpj_backward", "xgpj_final_state", "xgpj_version"]}
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    for prefix, header in (("xgj", "xgate_joint.h"), ("xgpj", "xgate_pos_joint.h")):
        assert _decl(header, prefix) == want[prefix]
        assert sorted(set(re.findall(r"\b(%s_[a-z_0-9]+)\b" % prefix, out))) == want[prefix]      # (no diag-only symbol in the product)
        for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
            if h != header:
                assert not re.search(r"\b%s_" % prefix, open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_versions_through_gcc_and_the_older_abis_unchanged(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_joint as nj
    from controllable_xgating_amd import _native_pos_joint as npj
    from controllable_xgating_amd import _native_pos_train as npt
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "xgate_joint.h"\n#include "xgate_pos_joint.h"\nint main(void) {\n'
                   '  printf("%d %d %d %d %zu %zu\\n", XGJ_VERSION, XGPJ_VERSION, XG_VERSION, XGPT_VERSION, sizeof(XgRun), sizeof(XgptRun));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    vj, vpj, vx, vpt, srun, sprun = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert vj == nj.XGJ_VERSION == nj.lib().xgj_version() == 1
    assert vpj == npj.XGPJ_VERSION == npj.lib().xgpj_version() == 1
    assert vx == nv.XG_VERSION == nv.lib().xg_version() and vpt == npt.XGPT_VERSION == npt.lib().xgpt_version()
    assert srun == ctypes.sizeof(nv.XgRun) and sprun == ctypes.sizeof(npt.XgptRun)
    assert nj.lib().xgj_last_kernel_width() == 0                  # nothing ran in this process


def _xgdims(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_xgj_caption_dpos_refuses_bad_arguments_without_a_gpu(built):
    """Every refusal is XG_EINVAL (-1) and comes before anything is enqueued: the pointers are fakes that are never dereferenced."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_joint as nj
    from controllable_xgating_amd import _native_ss as nss
    from controllable_xgating_amd import _native_train_video as ntv
    L = nj.lib()
    B = ctypes.byref
    d = pg.make_dims(**jo.CAP_TINY)
    dims = _xgdims(d)
    fake, big = 0x7F0000000000, 1 << 40
    x, run = nv.XgBatch(), nv.XgRun()

    def call(dm=dims, Q=0, form=nj.XGJ_FORM_XE, xb=x, r=run, ws=fake, n=big, out=fake):
        return L.xgj_caption_dpos(None, B(dm) if dm is not None else None, Q, form, B(xb) if xb is not None else None,
                                  B(r) if r is not None else None, ws, n, out)

    for kw in (dict(dm=None), dict(xb=None), dict(r=None), dict(ws=None), dict(out=None), dict(ws=fake + 4),
               dict(dm=_xgdims(d, B=0)), dict(dm=_xgdims(d, R=0)), dict(dm=_xgdims(d, L=-1)),
               dict(form=3), dict(form=-1),
               dict(Q=1), dict(Q=-1),                                                   # the plain loss has no rows per video
               dict(form=nj.XGJ_FORM_VIDEO, Q=0), dict(form=nj.XGJ_FORM_VIDEO, Q=-2),   # the per-video loss needs Q >= 1
               dict(form=nj.XGJ_FORM_SS, Q=-1),
               dict(form=nj.XGJ_FORM_VIDEO, Q=(1 << 20)),                               # too many rows
               dict(dm=_xgdims(d, B=(1 << 20) + 1))):
        assert call(**kw) == -1, kw
    # ws_bytes one below each form's size
    sizes = {(nj.XGJ_FORM_XE, 0): nv.lib().xg_workspace_bytes_mode(B(dims), 0),
             (nj.XGJ_FORM_SS, 0): nss.lib().xgss_workspace_bytes(B(dims), 0),
             (nj.XGJ_FORM_VIDEO, 3): ntv.lib().xgtv_workspace_bytes(B(dims), 3),
             (nj.XGJ_FORM_SS, 3): nss.lib().xgss_workspace_bytes(B(dims), 3)}
    for (form, Q), n in sizes.items():
        assert n > 0 and call(form=form, Q=Q, n=n - 1) == -1, (form, Q)
    assert sizes[(nj.XGJ_FORM_SS, 3)] > sizes[(nj.XGJ_FORM_VIDEO, 3)]
    # existing sizes stay what they were asked to stay: the plain forms share the standard workspace
    assert sizes[(nj.XGJ_FORM_XE, 0)] == sizes[(nj.XGJ_FORM_SS, 0)]


def _pos_fakes(d):
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_train as npt
    npos.lib()
    fake = 0x7F0000000000
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    run = npt.XgptRun(1, 0.0, 0, 0.1)
    return dims, P, run, fake


def test_xgpj_entry_points_refuse_bad_arguments_without_a_gpu(built):
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_joint as npj
    from controllable_xgating_amd import _native_pos_train as npt
    L = npj.lib()
    B = ctypes.byref
    d = po.make_dims(**jo.POS_TINY)
    dims, P, run, fake = _pos_fakes(d)
    T = d.L + 1
    need = npt.lib().xgpt_workspace_bytes(B(dims))
    assert need > 0
    # xgpj_final_state
    fs = lambda dm=dims, Tp=T, ws=fake, n=need, out=fake: L.xgpj_final_state(None, B(dm) if dm is not None else None, Tp, ws, n, out)   # noqa: E731
    for kw in (dict(dm=None), dict(Tp=0), dict(Tp=T + 1), dict(Tp=-3), dict(ws=None), dict(out=None),
               dict(dm=npos.XgpDims(0, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, T))):
        assert fs(**kw) == -1, kw
    assert fs(n=need - 1) == -4 and fs(n=0) == -4
    # xgpj_backward: xgpt_backward's gates, then "at least one of the two gradients"
    def bw(dm=dims, p=P, g=P, r=run, fr=fake, fo=fake, fm=fake, Tp=T, dl=fake, ws=fake, n=need, dp=fake):      # noqa: E306
        return L.xgpj_backward(None, B(dm), B(p) if p is not None else None, B(g) if g is not None else None,
                               B(r) if r is not None else None, fr, fo, fm, Tp, dl, ws, n, dp)
    holes = npos.XgpParams(*([fake] * (len(npos.PARAM_NAMES) - 1) + [None]))
    for kw in (dict(g=None), dict(g=holes), dict(p=None), dict(r=None), dict(r=npt.XgptRun(1, 1.0, 0, 0.1)), dict(Tp=0), dict(Tp=T + 1),
               dict(fr=None), dict(fo=None), dict(fm=None), dict(ws=None), dict(dl=None, dp=None)):
        assert bw(**kw) == -1, kw
    assert bw(n=need - 1) == -4 and bw(n=need - 1, dl=None) == -4
    # the same calls through xgpt_backward give the same codes (it still refuses a NULL dlogp)
    bt = lambda Tp=T, dl=fake, n=need: npt.lib().xgpt_backward(None, B(dims), B(P), B(P), B(run), fake, fake, fake, Tp, dl, fake, n)     # noqa: E731
    assert bt(Tp=0) == -1 and bt(dl=None) == -1 and bt(n=need - 1) == -4


def test_python_surface_refusals_that_need_no_gpu():
    import argparse
    from controllable_xgating_amd import JointTrainer, SAModel, make_opt
    from controllable_xgating_amd.pos import PosModel
    dc, dp = pg.make_dims(**jo.CAP_TINY), po.make_dims(**jo.POS_TINY)
    popt = lambda d: argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1,      # noqa: E731
                                        drop_prob_lm=0.0, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)
    pm = PosModel(popt(dp._replace(R=32)))
    cm = SAModel(make_opt(dc))
    opt = argparse.Namespace(learning_rate=1e-3, grad_clip=0.1, learning_rate_decay_start=-1)
    with pytest.raises(ValueError, match="rnn_size"):
        JointTrainer(cm, pm, opt)
    pm = PosModel(popt(dp)).eval()
    t = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="sample_forced"):
        pm(t, t, t, None, None, t, t, return_pos_feats=True)
