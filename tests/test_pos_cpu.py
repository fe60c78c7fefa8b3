"""CPU checks of the POS sequence generator: the tests-side oracle against the reference's own outputs (tests/golden/pos_*.npz), the
state_dict contract, the C ABI of include/xgate_pos.h (exports, struct sizes, parameter order, error codes without a GPU) and the
target preparation.  No compute on a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pos_oracle as po
from tests.util import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = list(po.GOLDEN_CASES)


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def load_case(name):
    cfg, kw, eos = po.GOLDEN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    g = dict(np.load(os.path.join(GOLD, "pos_%s.npz" % name)))
    return d, po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **kw), g


def make_opt(d, drop_prob_lm=0.0):
    import argparse
    return argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1,
                              drop_prob_lm=drop_prob_lm, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_goldens(name):
    d, P, run, x, g = load_case(name)
    P, run = po.to_torch(P), po.to_torch(run)
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    assert np.array_equal(cap_r.numpy(), g["cap_r"]) and np.array_equal(new_mask.numpy(), g["new_mask"])
    out = po.forward_tf(P, run, fr, fo, fm, cap_r, new_mask)
    assert out.shape[1] == int(g["tf_T"])
    np.testing.assert_allclose(out.numpy(), g["tf_logp"], atol=2e-5)
    if "loss" in g:
        loss = po.criterion(out, cap_r, new_mask, torch.from_numpy(x["class_mask"]))
        assert abs(float(loss) - float(g["loss"])) < 1e-5
    seq, slp, states, masks, _ = po.sample_greedy(P, run, fr, fo, fm, d.L)
    assert seq.shape[1] == int(g["n"])
    assert np.array_equal(seq.numpy(), g["seq"])
    np.testing.assert_allclose(slp.numpy(), g["seqLogprobs"], atol=2e-5)
    np.testing.assert_allclose(states.numpy()[:, :, :g["states"].shape[2]], g["states"], atol=2e-5)
    np.testing.assert_allclose(states.numpy()[:, -1], g["pos_feat"], atol=2e-5)
    assert np.array_equal(masks.numpy(), g["masks"])


def test_golden_cases_cover_the_early_exits():
    _, _, _, _, g = load_case("eos")
    ended = (g["seq"] == 0).any(1)
    assert int(g["n"]) < 12 and ended.any() and not ended.all()
    assert g["margin"][g["alive"]].min() >= 1e-3
    _, _, _, x, g = load_case("tfzero")
    assert int(g["tf_T"]) < g["cap_r"].shape[1] and "loss" not in g
    _, _, _, x, g = load_case("ragged")
    assert (x["feat_mask"] == 0).any() and len(set(g["new_mask"].sum(1).tolist())) > 2


def test_state_dict_matches_the_reference_and_loads_strict():
    from controllable_xgating_amd.pos import PosModel
    d, P, run, _, g = load_case("tiny")
    m = PosModel(make_opt(d))
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["keys"]) == po.state_dict_keys(d)
    assert len(sd) == 43
    for k, s in zip(g["keys"], g["shapes"]):
        shp = tuple(int(v) for v in s.split(",")) if s else ()
        assert tuple(sd[k].shape) == shp, k
    ref = {k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}
    m.load_state_dict(ref, strict=True)
    assert torch.equal(m.lstmcore.h2a.weight, ref["lstmcore.h2a.weight"])
    assert [n for n, _ in m.named_parameters()] == list(po.param_shapes(d))


def _pos_header():
    txt = open(os.path.join(ROOT, "include", "xgate_pos.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_xgp_function(built):
    syms = sorted(set(re.findall(r"\b(xgp_[a-z_0-9]+)\s*\(", _pos_header())))
    assert len(syms) == 8
    lib = ctypes.CDLL(built)
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s


def test_struct_sizes_and_parameter_order(built, tmp_path):
    from controllable_xgating_amd import _native_pos as npos
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_pos.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d\\n", sizeof(XgpDims), sizeof(XgpParams), XGP_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, ver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = npos.lib()
    assert ver == npos.XGP_VERSION == L.xgp_version()
    assert sd == ctypes.sizeof(npos.XgpDims) and sp == ctypes.sizeof(npos.XgpParams)
    d = po.make_dims(**po.POS_CFG["c1"])
    assert npos.PARAM_NAMES == list(po.param_shapes(d))
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    for i, (n, shp) in enumerate(po.param_shapes(d).items()):
        k = ctypes.c_int64()
        assert L.xgp_param_numel(ctypes.byref(dims), i, ctypes.byref(k)) == 0
        assert k.value == int(np.prod(shp)), n
    assert L.xgp_param_name(len(npos.PARAM_NAMES)) is None
    assert L.xgp_workspace_bytes(ctypes.byref(dims)) > 0


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    L = npos.lib()
    d = po.make_dims(**po.POS_CFG["tiny"])
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    bad = npos.XgpDims(0, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    assert L.xgp_workspace_bytes(ctypes.byref(bad)) == 0
    k = ctypes.c_int64()
    assert L.xgp_param_numel(ctypes.byref(dims), -1, ctypes.byref(k)) == -1
    assert L.xgp_param_numel(ctypes.byref(bad), 0, ctypes.byref(k)) == -1
    P = npos.XgpParams(*([None] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState()
    assert L.xgp_encoder_fwd(None, ctypes.byref(dims), ctypes.byref(P), ctypes.byref(bn), None, None, None, None, None, 0) == -1
    assert L.xgp_forward_tf(None, ctypes.byref(dims), None, None, None, None, None, None, None, None, None, None, 0) == -1
    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    assert L.xgp_sample_greedy(None, ctypes.byref(dims), ctypes.byref(P), ctypes.byref(bn), fake, fake, fake, fake, fake, fake,
                               fake, fake, fake, 8) == -4
    one = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, 1)           # a rollout needs T >= 2
    assert L.xgp_sample_greedy(None, ctypes.byref(one), ctypes.byref(P), ctypes.byref(bn), fake, fake, fake, fake, fake, fake,
                               fake, fake, fake, 1 << 40) == -1


def test_prepare_pos_targets_matches_the_reference_roll_and_new_mask():
    from controllable_xgating_amd.pos import prepare_pos_targets
    for name in ("tiny", "ragged", "tfzero"):
        _, _, _, x, g = load_case(name)
        cap, cm = torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"])
        rolled, new_mask = prepare_pos_targets(cap, cm)
        # starttrain_trainpos.py:132-136, literally
        ref_r = torch.cat([cap[:, -1:], cap[:, :-1]], dim=-1)
        ref_m = torch.zeros_like(cm)
        for i in range(cm.size(0)):
            index = np.argwhere(cm[i, :] != 0)[0][-1]
            ref_m[i, :index + 1] = 1.0
        assert torch.equal(rolled, ref_r) and torch.equal(new_mask, ref_m)
        assert np.array_equal(new_mask.numpy(), g["new_mask"])


def test_unsupported_modes_raise_not_implemented():
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(make_opt(d))
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    args = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    with pytest.raises(NotImplementedError):
        m.sample(*args, {"sample_max": 1})               # train mode (a fresh module)
    m.eval()
    with pytest.raises(NotImplementedError):
        m.sample(*args, {"beam_size": 3})
    with pytest.raises(NotImplementedError):
        m.sample(*args, {"sample_max": 0})
    m.train()
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    with pytest.raises(NotImplementedError):
        m(*args, None, None, cap_r, new_mask)
