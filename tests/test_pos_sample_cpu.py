"""CPU checks of sampled POS templates: the sampled-rollout oracle (tests/pos_sample_oracle.py) against the reference's greedy
fixtures at a low temperature, against the forced oracle fed its own draws, and at the edge uniforms; the C ABI of
include/xgate_pos_sample.h (exports, version, struct sizes, error codes without a GPU); control.first_occurrences; and the
refusals of PosModel.sample_templates.  No compute on a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import pos_control_oracle as pco
from tests import pos_oracle as po
from tests import pos_sample_oracle as pso
from tests.util import ROOT

FIXTURES = ("tiny", "c1", "ragged", "eos")


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _cpu_inputs(x):
    return [torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


def _cpu_sampled(d, P, run, x, u, temperature):
    return pso.sample_templates(po.to_torch(P), po.to_torch(run), *_cpu_inputs(x), u, d.L, temperature)


@pytest.mark.parametrize("name", FIXTURES)
def test_low_temperature_oracle_reproduces_the_greedy_goldens(name):
    """temperature 1e-5 with every uniform 0.5: the fixtures' smallest top-2 margin is 2.6e-4, so a runner-up weighs e^-26 and
    the draw is the argmax."""
    d, P, run, x, g = pco.load_case(name)
    o = _cpu_sampled(d, P, run, x, torch.full((d.B, 1, d.L), 0.5), 1e-5)
    n = int(g["n"])
    assert o["n"] == n
    tm = o["templates"][:, 0].numpy()
    assert np.array_equal(tm[:, :n], g["seq"]) and (tm[:, n:] == 0).all()
    assert np.array_equal(o["masks"][:, 0, :n + 1].numpy(), g["masks"])


@pytest.mark.parametrize("temperature", [0.7, 1.0, 1.3])
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_draws_fed_to_the_forced_oracle_give_the_same_rollout(name, temperature):
    d, P, run, x, _ = pco.load_case(name)
    u = torch.from_numpy(pg.uniform("pos_sample_u", (d.B, 5, d.L), 11))
    o = _cpu_sampled(d, P, run, x, u, temperature)
    tm = o["templates"]
    assert tm.dtype == torch.int64 and tm.shape == (d.B, 5, d.L) and int(tm.min()) >= 0 and int(tm.max()) < d.C
    alive = torch.cat([torch.ones(d.B, 5, 1, dtype=torch.bool), (tm[:, :, :-1] > 0).cumprod(2).bool()], 2)
    assert (tm[~alive] == 0).all()                               # zero from a row's first 0 onwards
    f = pco.sample_forced(po.to_torch(P), po.to_torch(run), *_cpu_inputs(x), tm, d.L)
    for k in ("tag_logp", "masks", "states", "pos_feats"):
        assert torch.equal(o[k], f[k]), k
    assert o["n"] == f["n"]
    lp = o["tag_logp"]
    assert (lp[alive] < 0).all() and (lp[~alive] == 0).all()


@pytest.mark.parametrize("name", ["tiny", "eos"])
def test_oracle_edge_uniforms(name):
    d, P, run, x, _ = pco.load_case(name)
    o = _cpu_sampled(d, P, run, x, torch.zeros(d.B, 2, d.L), 1.0)
    assert (o["templates"] == 0).all() and o["n"] == 0
    assert (o["masks"][:, :, 0] == 1).all() and (o["masks"][:, :, 1:] == 0).all()
    assert (o["tag_logp"][:, :, 0] < 0).all() and (o["tag_logp"][:, :, 1:] == 0).all()
    o = _cpu_sampled(d, P, run, x, torch.ones(d.B, 2, d.L), 1.0)
    assert (o["templates"] == d.C - 1).all() and o["n"] == d.L
    assert (o["masks"] == 1).all() and (o["tag_logp"] < 0).all()


def _sample_header():
    txt = open(os.path.join(ROOT, "include", "xgate_pos_sample.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgps_[a-z_0-9]+)\s*\(", _sample_header())))
    assert syms == ["xgps_sample_templates", "xgps_version", "xgps_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\b(xgps_[a-z_0-9]+)\b", out)))
    assert exported == syms
    # the sibling headers declare none of them: the new entry points live in their own header
    for h in ("xgate_pos.h", "xgate_pos_control.h", "xgate_pos_train.h", "xgate.h"):
        assert "xgps_" not in open(os.path.join(ROOT, "include", h)).read(), h


def test_version_and_struct_sizes_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_control as npc
    from controllable_xgating_amd import _native_pos_sample as nps
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_pos_sample.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d\\n", sizeof(XgpDims), sizeof(XgpParams), sizeof(XgBnState), XGPS_VERSION, '
                   'XGPC_VERSION, XGP_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, sb, ver, cver, pver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = nps.lib()
    assert ver == nps.XGPS_VERSION == L.xgps_version() == 1
    assert cver == npc.XGPC_VERSION and pver == npos.XGP_VERSION
    assert sd == ctypes.sizeof(npos.XgpDims) and sp == ctypes.sizeof(npos.XgpParams) and sb == ctypes.sizeof(nv.XgBnState)


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_sample as nps
    L = nps.lib()
    d = po.make_dims(**po.POS_CFG["tiny"])
    B = ctypes.byref
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    sizes = [L.xgps_workspace_bytes(B(dims), S) for S in (1, 2, 3, 8, 33)]
    assert sizes[0] > npos.lib().xgp_workspace_bytes(B(dims)) > 0
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                       # grows with S
    assert L.xgps_workspace_bytes(B(dims), 0) == 0 and L.xgps_workspace_bytes(B(dims), -1) == 0
    bad = npos.XgpDims(0, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    one = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, 1)            # a rollout needs T >= 2
    assert L.xgps_workspace_bytes(B(bad), 2) == 0 and L.xgps_workspace_bytes(B(one), 2) == 0
    assert L.xgps_workspace_bytes(B(dims), 1 << 20) == 0                      # B * S rows beyond 32-bit offsets
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def call(dm=dims, S=2, temp=1.0, p=P, b=bn, ptrs=None, ws=fake, nbytes=big):
        a = [fake] * 10 if ptrs is None else ptrs      # fr, fo, fm, uniforms, templates, tag_logp, states, masks, pos_feats, n_out
        return L.xgps_sample_templates(None, B(dm), S, temp, None if p is None else B(p), None if b is None else B(b), a[0], a[1],
                                       a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4
    assert call(nbytes=sizes[1] - 1) == -4
    assert call(S=3, nbytes=sizes[1]) == -4              # the workspace of S = 2 does not serve S = 3
    assert call(temp=0.25, nbytes=8) == -4 and call(temp=1e-5, nbytes=8) == -4 and call(temp=100.0, nbytes=8) == -4
    for t in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(temp=t) == -1, t
    assert call(S=0) == -1 and call(S=-2) == -1
    assert call(dm=bad) == -1 and call(dm=one) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(ws=None) == -1
    assert call(p=npos.XgpParams(*([fake] * (len(npos.PARAM_NAMES) - 1) + [None]))) == -1
    for i in range(10):
        if i == 6:
            continue                                    # states may be NULL: with every other pointer set the next check decides
        ptrs = [fake] * 10
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1, i
    ptrs = [fake] * 10
    ptrs[6] = None
    assert call(ptrs=ptrs, nbytes=8) == -4


def test_first_occurrences_on_hand_made_templates():
    from controllable_xgating_amd import first_occurrences
    t = torch.tensor([[[1, 2, 0], [1, 2, 0], [1, 0, 0], [1, 2, 0], [1, 0, 0]],
                      [[0, 0, 0], [3, 0, 0], [0, 0, 0], [3, 1, 0], [3, 0, 0]]])
    f = first_occurrences(t)
    assert f.dtype == torch.bool and f.shape == (2, 5)
    assert f.tolist() == [[True, False, True, False, False], [True, True, False, True, False]]
    assert first_occurrences(t[:, :1]).tolist() == [[True], [True]]
    # templates of DIFFERENT videos never shadow each other
    assert first_occurrences(torch.tensor([[[1, 2]], [[1, 2]]])).tolist() == [[True], [True]]
    with pytest.raises(ValueError):
        first_occurrences(torch.zeros(2, 3, dtype=torch.int64))


def test_train_mode_and_cpu_tensors_raise(built):
    from controllable_xgating_amd import XgError
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(pco.make_opt(d))                           # a fresh module is in train mode
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    with pytest.raises(NotImplementedError):
        m.sample_templates(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], 2)
    m.eval()
    with pytest.raises(XgError):
        m.sample_templates(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], 2)
    # PosModel.sample keeps refusing sample_max = 0: the sampled rollout has its own entry point
    with pytest.raises(NotImplementedError):
        m.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], {"sample_max": 0})


def test_replay_cases_reach_the_branches_they_name():
    """The cases of tests/test_gpu_pos_sample.py's float64 replay, against xg_pos.hip's selections restated here."""
    from controllable_xgating_amd import _native_pos_control as npc
    from tests.test_gpu_pos_sample import CASES, GROUP
    assert npc.XGPC_TEMPLATE_GROUP == GROUP
    d, S = CASES["tiny_s3"]
    assert d == po.POS_CFG["tiny"] and d["B"] * S == 15 and 1 < S < GROUP
    d, S = CASES["a_r_odd"]
    assert (d["B"], d["K"], d["R"], d["A"]) == (3, 5, 22, 38) and d["A"] % 4 and d["R"] % 4      # scalar loads; the staged product
    d, S = CASES["group_plus_1"]
    assert S == 5 and S % GROUP == 1 and S > GROUP                                              # a full group and a partial one
    # pos_cell_head_rows_kernel<true>: C <= 64 one lane per category (scan + ballot), serial beyond
    assert [CASES[k][0]["C"] for k in ("c64", "c65", "c130")] == [64, 65, 130]
    for k in ("c64", "c65", "c130"):
        d, S = CASES[k]
        assert (d["B"], d["K"], d["R"], d["A"]) == (2, 5, 40, 52)
    assert all(dd["C"] <= 64 for k, (dd, _) in CASES.items() if k not in ("c65", "c130"))
    d, S = CASES["rows_297"]
    assert d["B"] * S == 297 and S % GROUP                                                      # > 256 rows: n_out's second pass
    d, S = CASES["c1_s8"]
    assert d == po.POS_CFG["c1"] and S == 8 and S % GROUP == 0

    def group_lds(d, G):                                         # xg_pos.hip: attn_group_lds
        nsplit = min(max(1024 // d["R"], 1), d["K"])
        r4 = lambda v: (v + 3) // 4 * 4
        return 4 * (r4(G * max(d["A"], nsplit * d["R"])) + r4(d["A"]) + G * d["K"])

    for name, (d, S) in CASES.items():                           # every case runs pos_attn_group_kernel<4>: S > 1, LDS within 64 KiB
        assert S > 1 and group_lds(d, GROUP) <= 64 * 1024, name
        assert 4 * (d["R"] + 2 * d["C"]) <= 64 * 1024, name      # the sampled cell's LDS: h, the logits, the serial head's weights
