"""CPU checks of controlled POS generation: the forced-rollout oracle (tests/pos_control_oracle.py) fed each reference fixture's own
greedy tokens against that fixture (tests/golden/pos_*.npz), the semantics of the end tag, the C ABI of
include/xgate_pos_control.h (exports, version, struct sizes, error codes without a GPU) and control.pad_templates.  No compute on a
GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pos_control_oracle as pco
from tests import pos_oracle as po
from tests.util import ROOT



@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _cpu_oracle(d, P, run, x, tm):
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    return pco.sample_forced(po.to_torch(P), po.to_torch(run), fr, fo, fm, tm, d.L)


@pytest.mark.parametrize("name", list(po.GOLDEN_CASES))
def test_forced_oracle_on_golden_tokens_matches_reference_goldens(name):
    d, P, run, x, g = pco.load_case(name)
    tm, comparable = pco.golden_template(d, g)
    o = _cpu_oracle(d, P, run, x, tm)
    n = int(g["n"])
    assert o["n"] == n
    cols = g["states"].shape[2]
    np.testing.assert_allclose(o["states"][:, 0, :n + 1, :cols].numpy(), g["states"], atol=2e-5)
    assert np.array_equal(o["masks"][:, 0, :n + 1].numpy(), g["masks"])
    np.testing.assert_allclose(o["pos_feats"].numpy(), g["pos_feat"], atol=2e-5)
    np.testing.assert_allclose(o["states"][:, 0, n].numpy(), o["pos_feats"].numpy(), atol=0)     # finished rows hold
    lp = o["tag_logp"][:, 0, :n].numpy()
    np.testing.assert_allclose(lp[comparable], g["seqLogprobs"][comparable], atol=2e-5)
    assert (lp[~comparable] == 0).all()
    if name == "eos":
        assert 0.7 < comparable.mean() < 0.75
    else:
        assert comparable.all()


def test_tag_logp_is_zero_after_the_finish_and_later_tags_change_nothing():
    d, P, run, x, _ = pco.load_case("ragged")
    tm, lens = pco.seeded_templates(d.B, 3, d.L, d.C, seed=3)
    o = _cpu_oracle(d, P, run, x, tm)
    pos = np.arange(d.L)[None, None, :]
    after = pos > lens[:, :, None]                              # position lens is the end tag: it still counts
    lp = o["tag_logp"].numpy()
    assert (lp[after] == 0).all() and (lp[~after] < 0).all()
    assert lens.reshape(-1)[0] == 0 and lens.reshape(-1)[1] == d.L
    clean = tm.clone()
    clean[torch.from_numpy(pos >= lens[:, :, None])] = 0        # the junk after each first 0 removed
    assert not torch.equal(clean, tm)
    o2 = _cpu_oracle(d, P, run, x, clean)
    for k in ("tag_logp", "states", "masks", "pos_feats"):
        assert torch.equal(o[k], o2[k]), k
    assert o["n"] == o2["n"] == d.L
    # an all-empty batch: n = 0 and pos_feats is the state after BOS
    o3 = _cpu_oracle(d, P, run, x, torch.zeros_like(tm))
    assert o3["n"] == 0
    assert torch.equal(o3["pos_feats"].reshape(d.B, 3, -1), o3["states"][:, :, 0])
    assert (o3["masks"][:, :, 0] == 1).all() and (o3["masks"][:, :, 1:] == 0).all()


def _control_header():
    txt = open(os.path.join(ROOT, "include", "xgate_pos_control.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgpc_[a-z_0-9]+)\s*\(", _control_header())))
    assert syms == ["xgpc_sample_forced", "xgpc_version", "xgpc_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\b(xgpc_[a-z_0-9]+)\b", out)))
    assert exported == syms
    # the sibling header still declares its 8 entry points: the new ones live in their own header
    pos = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xgate_pos.h")).read(), flags=re.S)
    assert "xgpc_" not in pos


def test_version_and_struct_sizes_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_control as npc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_pos_control.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d\\n", sizeof(XgpDims), sizeof(XgpParams), sizeof(XgBnState), XGPC_VERSION, '
                   'XGP_VERSION, XGPC_TEMPLATE_GROUP);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, sb, ver, pver, grp = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    from controllable_xgating_amd import _native as nv
    L = npc.lib()
    assert ver == npc.XGPC_VERSION == L.xgpc_version()
    assert pver == npos.XGP_VERSION
    assert grp == npc.XGPC_TEMPLATE_GROUP
    assert sd == ctypes.sizeof(npos.XgpDims) and sp == ctypes.sizeof(npos.XgpParams) and sb == ctypes.sizeof(nv.XgBnState)


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_control as npc
    L = npc.lib()
    d = po.make_dims(**po.POS_CFG["tiny"])
    B = ctypes.byref
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    sizes = [L.xgpc_workspace_bytes(B(dims), S) for S in (1, 2, 3, 8, 33)]
    assert sizes[0] > npos.lib().xgp_workspace_bytes(B(dims)) > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                       # grows with S
    assert L.xgpc_workspace_bytes(B(dims), 0) == 0 and L.xgpc_workspace_bytes(B(dims), -1) == 0
    bad = npos.XgpDims(0, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    one = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, 1)            # a rollout needs T >= 2
    assert L.xgpc_workspace_bytes(B(bad), 2) == 0 and L.xgpc_workspace_bytes(B(one), 2) == 0
    assert L.xgpc_workspace_bytes(B(dims), 1 << 20) == 0                      # B * S rows beyond 32-bit offsets
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def call(dm=dims, S=2, p=P, b=bn, ptrs=None, ws=fake, nbytes=big):
        a = [fake] * 9 if ptrs is None else ptrs       # fr, fo, fm, templates, tag_logp, states, masks, pos_feats, n_out
        return L.xgpc_sample_forced(None, B(dm), S, None if p is None else B(p), None if b is None else B(b), a[0], a[1], a[2], a[3],
                                    a[4], a[5], a[6], a[7], a[8], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4
    assert call(nbytes=sizes[1] - 1) == -4
    assert call(S=3, nbytes=sizes[1]) == -4              # the workspace of S = 2 does not serve S = 3
    assert call(S=0) == -1 and call(S=-2) == -1
    assert call(dm=bad) == -1 and call(dm=one) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(ws=None) == -1
    assert call(p=npos.XgpParams(*([fake] * (len(npos.PARAM_NAMES) - 1) + [None]))) == -1
    for i in range(9):
        if i == 5:
            continue                                    # states may be NULL: with every other pointer set the next check decides
        ptrs = [fake] * 9
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1, i
    ptrs = [fake] * 9
    ptrs[5] = None
    assert call(ptrs=ptrs, nbytes=8) == -4


def test_pad_templates_pads_and_raises():
    from controllable_xgating_amd import pad_templates
    t = pad_templates([[[3, 1], []], [[2], [1, 1, 4]]], 4, 5)
    assert t.dtype == torch.int64 and t.shape == (2, 2, 4)
    assert t.tolist() == [[[3, 1, 0, 0], [0, 0, 0, 0]], [[2, 0, 0, 0], [1, 1, 4, 0]]]
    assert pad_templates([[3, 1], [2]], 4, 5).tolist() == [[[3, 1, 0, 0]], [[2, 0, 0, 0]]]          # (B, L'): S = 1
    assert pad_templates(np.array([[1, 2], [3, 0]]), 3, 5).tolist() == [[[1, 2, 0]], [[3, 0, 0]]]
    assert pad_templates(torch.tensor([[[1, 2, 3]]], dtype=torch.int32), 3, 5).tolist() == [[[1, 2, 3]]]
    for bad in ([[[5]]], [[[-1]]], [[1, 2, 3, 4, 1]], [[[1], [2]], [[1]]], [], np.array([[1, 7]]), torch.tensor([[[1, 2, 3, 4, 0]]]),
                np.array([[0.5]]), np.zeros((1, 1, 1, 1), np.int64)):
        with pytest.raises(ValueError):
            pad_templates(bad, 4, 5)


def test_train_mode_raises_not_implemented():
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(pco.make_opt(d))                           # a fresh module is in train mode
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    with pytest.raises(NotImplementedError):
        m.sample_forced(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], torch.zeros(d.B, d.L, dtype=torch.int64))
