"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every
symbol include/xgate.h declares; the Python mirror keeps the reference's state_dict contract.
No compute calls (there is no GPU here)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests.util import ROOT, CFG, header_symbols


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built)
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s


def test_version_strerror_and_param_table(built):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    assert L.xg_version() == 206 == nv.XG_VERSION
    assert L.xg_strerror(0) == b"ok"
    assert b"workspace" in L.xg_strerror(-4)
    d = pg.make_dims(**CFG["c1"])
    shapes = pg.param_shapes(d)
    assert nv.PARAM_NAMES == list(shapes.keys())          # ABI order == SURVEY Appendix B order
    dims = nv.XgDims(d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H, d.F1, d.F2, d.L + 1)
    tot = 0
    for i, n in enumerate(nv.PARAM_NAMES):
        k = ctypes.c_int64()
        assert L.xg_param_numel(ctypes.byref(dims), i, ctypes.byref(k)) == 0
        assert k.value == int(np.prod(shapes[n])), n
        tot += k.value
    assert tot == 36122159                                  # parameter count at V = 20000
    full = L.xg_workspace_bytes(ctypes.byref(dims))
    assert full > 0
    # only the bf16 mode carries the bf16 mirror region (a third of the full size)
    assert L.xg_workspace_bytes_mode(ctypes.byref(dims), 1) == full
    core = L.xg_workspace_bytes_mode(ctypes.byref(dims), 0)
    assert core == L.xg_workspace_bytes_mode(ctypes.byref(dims), 3) and 0.60 * full < core < 0.70 * full
    bad = nv.XgDims(0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert L.xg_workspace_bytes(ctypes.byref(bad)) == 0


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    assert L.xg_nll_fwd(None, None, None, None, None, 1, 1, 1, 0, None) == -1
    assert L.xg_clip_adam(None, 10, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0.1) == -1
    d = pg.make_dims(**CFG["tiny"])
    dims = nv.XgDims(d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H, d.F1, d.F2, d.L + 1)
    assert L.xg_vproj(None, ctypes.byref(dims), None, None, None, None) == -1


def test_state_dict_contract_matches_reference_names_and_shapes(built):
    from controllable_xgating_amd import SAModel, make_opt
    d = pg.make_dims(**CFG["tiny"])
    m = SAModel(make_opt(d))
    sd = m.state_dict()
    shapes = pg.param_shapes(d)
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    extra = set(sd) - set(shapes)
    assert all(("running_" in k) or ("num_batches_tracked" in k) for k in extra), extra
    assert [n for n, _ in m.named_parameters() if n not in shapes] == []
    # reference quirk: same-seeded sibling gates start identical
    assert torch.equal(sd["two_spatial_encoder.gate_rgb.gate.0.weight"], sd["two_spatial_encoder.gate_opfl.gate.0.weight"])
    assert float(sd["logit.bias"].abs().max()) == 0.0
    assert float(sd["embed.weight"].abs().max()) <= 0.1


def test_product_fails_loudly_without_library(built, tmp_path):
    code = ("import controllable_xgating_amd._native as nv; nv.LIB_PATH='/nonexistent/libxgate_hip.so'\n"
            "try:\n    nv.lib()\nexcept nv.XgError as e:\n    print('LOUD', e)\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert "LOUD" in out.stdout and "no CPU / PyTorch fallback" in out.stdout


def test_cpu_tensors_are_rejected(built):
    from controllable_xgating_amd import SAModel, make_opt, XgError
    d = pg.make_dims(**CFG["tiny"])
    m = SAModel(make_opt(d))
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    with pytest.raises(XgError):
        m(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "controllable_xgating_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), f


_STRUCTS = ("XgDims", "XgParams", "XgBnState", "XgBatch", "XgRun")


def _header_sizes(tmp_path):
    """sizeof of the five ABI structs (and XG_VERSION) as a C99 compiler sees include/xgate.h."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in _STRUCTS) +
                   '  printf("XG_VERSION %d\\n", XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def _integration_stub():
    """The struct mirror a maintainer is told to paste, executed without loading any library."""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a = txt.index("# --- struct mirror of include/xgate.h")
    b = txt.index("# --- end of the struct mirror ---")
    ns = {"C": ctypes}
    exec(txt[a:b], ns)
    return ns


def test_struct_sizes_agree_between_header_binding_and_integration_stub(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    hdr = _header_sizes(tmp_path)
    assert hdr["XG_VERSION"] == nv.XG_VERSION == L.xg_version()
    mine = {"XgDims": nv.XgDims, "XgParams": nv.XgParams, "XgBnState": nv.XgBnState, "XgBatch": nv.XgBatch, "XgRun": nv.XgRun}
    stub = _integration_stub()
    theirs = {"XgDims": stub["XgDims"], "XgParams": stub["XgParams"], "XgBnState": stub["XgBn"], "XgBatch": stub["XgBatch"],
              "XgRun": stub["XgRun"]}
    for n in _STRUCTS:
        assert ctypes.sizeof(mine[n]) == hdr[n], (n, ctypes.sizeof(mine[n]), hdr[n])
        assert ctypes.sizeof(theirs[n]) == hdr[n], ("INTEGRATION.md stub", n, ctypes.sizeof(theirs[n]), hdr[n])
    assert stub["XG_VERSION"] == hdr["XG_VERSION"] and stub["N_PARAMS"] == L.xg_param_count()
    # field names and order of the stub's XgRun == the binding's (same header fields, in order)
    assert [f[0] for f in stub["XgRun"]._fields_] == [f[0] for f in nv.XgRun._fields_]
    hdr_txt = open(os.path.join(ROOT, "include", "xgate.h")).read()
    run_body = hdr_txt[hdr_txt.index("typedef struct XgRun {"):hdr_txt.index("} XgRun;")]
    pos = [run_body.index(f[0]) for f in nv.XgRun._fields_]
    assert pos == sorted(pos)
    # the library's own check: right sizes pass, a stale (12-field, 64-byte) XgRun or an old version number does not
    sz = [hdr[n] for n in _STRUCTS]
    assert L.xg_abi_check(hdr["XG_VERSION"], *sz) == 0
    assert L.xg_abi_check(hdr["XG_VERSION"], *sz[:4], 64) == -1
    assert L.xg_abi_check(hdr["XG_VERSION"] - 1, *sz) == -1


def test_product_library_has_no_low_lane_operand_select_on_packed_fp32(built):
    """docs/pkfma_hazard.md: `v_pk_fma_f32 ... op_sel:[0,1,0]` (the low lane takes the HIGH register of a pair) lost its low-lane
    product in lanes 48-63 now and then beside split-bf16 tiles.  The attention context loop is pinned to v_fmac_f32 and the library is
    built with -fno-slp-vectorize; this test reads the gfx950 code objects of the built product library back and fails on any
    packed-fp32 instruction with an `op_sel:` modifier, wherever a later compiler or a new float2 loop puts one."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_packed_opsel as chk
    if not os.path.exists(chk.OBJDUMP):
        pytest.skip("llvm-objdump not in this image")
    objs = chk.code_objects(built)
    assert len(objs) >= 8, "no gfx950 code objects found in %s" % built      # one per .hip translation unit
    low = [(sym, ins) for sym, ins in chk.packed_opsel_sites(built) if re.search(r"\bop_sel:\[", ins)]
    assert not low, "packed fp32 with low-lane operand select in the product library: %s" % low[:4]


# ---- the argument gate of every workspace-taking entry point (no call below gets past it, so nothing is enqueued)
_FAKE = 0x7F0000000000                # stands in for every pointer: 256-byte aligned, never dereferenced
_HUGE = 1 << 40
_DIMS = ("B", "K", "R", "A", "E", "V", "C", "H", "F1", "F2", "T")
# arguments in ABI order.  d / d2 / d1: XgDims; p / g: XgParams; bn, x, run: the structs; ws* / bytes*: a workspace and its size;
# a name of _SCALARS: that value; every other name: a device pointer
_ENTRY = {
    "xg_encoder_fwd": "stream d p bn x run ws bytes V",
    "xg_encoder_bwd": "stream d p g x run ws bytes dV",
    "xg_init_hidden": "stream d p V feat_mask ws bytes state",
    "xg_step_fwd": "stream d p tokens xt_mask V vproj pos_feats run step ws bytes state logp alpha",
    "xg_step_bwd": "stream d p g tokens xt_mask V vproj pos_feats run step ws bytes state_new dstate_new dstate dV_out dvproj dpos",
    "xg_forward_xe": "stream d p bn x run ws bytes logp cat_logp",
    "xg_backward_xe": "stream d p g x run ws bytes dlogp dcat_logp",
    "xg_forward_ss": "stream d p bn x run ss_prob u_sel u_tok ws bytes logp cat_logp",
    "xg_backward_ss": "stream d p g x run ws bytes dlogp dcat_logp",
    "xg_xe_loss_fwd": "stream d p bn x cap_classes class_mask weight_class run ws bytes losses",
    "xg_xe_loss_bwd": "stream d p g x cap_classes class_mask weight_class dloss run ws bytes",
    "xg_rollout": "stream d p bn x run mode uniforms forced temperature ws bytes seq seq_logp n_steps",
    "xg_rollout_pair": "stream d2 p bn x run n_sample uniforms temperature ws2 bytes2 seq seq_logp n_steps",
    "xg_rollout_compact": "stream d2 ws2 bytes2 d1 ws1 bytes1",
    "xg_rollout_pair_compact": "stream d2 p bn x run n_sample uniforms temperature ws2 bytes2 d1 ws1 bytes1 seq seq_logp n_steps",
    "xg_rollout_pair_videos": "stream d2 p bn x run uniforms temperature ws2 bytes2 d1 ws1 bytes1 compact seq seq_logp n_steps",
    "xg_rollout_bwd": "stream d p g x run ws bytes dseq_logp",
}
_SCALARS = dict(step=0, ss_prob=0.5, weight_class=1.0, mode=0, temperature=1.0, n_sample=5, compact=1)
# what each entry point tests after its workspace(s): (arguments, XgBatch fields) that must not be NULL
_REQUIRED = {
    "xg_encoder_fwd": ("p x run V", "feats_rgb feats_opfl feat_mask"),
    "xg_encoder_bwd": ("p g x run dV", ""),
    "xg_init_hidden": ("p V feat_mask state", ""),
    "xg_step_fwd": ("p tokens V vproj pos_feats run state", ""),
    "xg_step_bwd": ("p g tokens V vproj pos_feats run state_new dstate_new dstate", ""),
    "xg_forward_xe": ("p x run logp", "seq seq_mask pos_feats"),
    "xg_backward_xe": ("p g x run", "seq seq_mask"),
    "xg_forward_ss": ("p x run logp u_sel u_tok", "seq seq_mask pos_feats"),      # (u_*: run.train and ss_prob > 0 here)
    "xg_backward_ss": ("p g x run", "seq seq_mask"),
    "xg_xe_loss_fwd": ("p x run losses", "seq seq_mask pos_feats"),
    "xg_xe_loss_bwd": ("p g x run", "seq seq_mask"),
    "xg_rollout": ("p x run seq seq_logp n_steps", "pos_feats"),
    "xg_rollout_pair": ("p x run seq seq_logp n_steps uniforms", "pos_feats"),
    "xg_rollout_compact": ("", ""),
    "xg_rollout_pair_compact": ("p x run seq seq_logp n_steps uniforms", "pos_feats"),
    "xg_rollout_pair_videos": ("p x run seq seq_logp n_steps uniforms", "pos_feats feats_rgb feats_opfl feat_mask"),
    "xg_rollout_bwd": ("p g x run dseq_logp", ""),
}


def _gate_call(nv, L, name, dims=None, batch=None, **over):
    """Call `name` with fake pointers everywhere.  dims: {"d": {"B": 0}} changes fields of that XgDims argument; batch: fields of the
    XgBatch; over: an argument by name (None = NULL)."""
    t = pg.make_dims(**CFG["tiny"])
    keep, args = [], []
    for a in _ENTRY[name].split():
        if a in over:
            v = over[a]
        elif a == "stream":
            v = None
        elif a in ("d", "d1", "d2"):
            f = dict(zip(_DIMS, (t.B, t.K, t.R, t.A, t.E, t.V, t.C, t.H, t.F1, t.F2, t.L + 1)))
            if a == "d2":
                f["B"] = 2 * t.B
            f.update((dims or {}).get(a, {}))
            v = nv.XgDims(*[f[k] for k in _DIMS])
        elif a in ("p", "g"):
            v = nv.XgParams()
            for fld, _ in v._fields_:
                setattr(v, fld, _FAKE)
        elif a == "bn":
            v = nv.XgBnState(_FAKE, _FAKE, _FAKE, _FAKE)
        elif a == "x":
            f = dict.fromkeys((n for n, _ in nv.XgBatch._fields_), _FAKE)
            f.update(batch or {})
            v = nv.XgBatch(*[f[n] for n, _ in nv.XgBatch._fields_])
        elif a == "run":
            v = nv.XgRun(train=1, drop_p=0.0, seed=1, save=0, bn_momentum=0.1, bn_eps=1e-5)
        elif a.startswith("ws"):
            v = _FAKE + (_HUGE << 1 if a == "ws1" else 0)
        elif a.startswith("bytes"):
            v = _HUGE
        elif a in _SCALARS:
            v = _SCALARS[a]
        else:
            v = _FAKE
        if isinstance(v, ctypes.Structure):
            keep.append(v)
            v = ctypes.byref(v)
        args.append(v)
    return getattr(L, name)(*args)


def test_entry_points_gate_their_arguments_without_a_gpu(built):
    """Every workspace-taking export answers in this order: bad dims or a NULL workspace -1, a workspace that is too small -4,
    a misaligned workspace -1, and only then its own pointer and scalar tests -1.  Every call here carries one such defect."""
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    assert set(_ENTRY) == set(_REQUIRED) and all(hasattr(L, n) for n in _ENTRY)
    B = CFG["tiny"]["B"]
    for name, spec in _ENTRY.items():
        names = spec.split()

        def call(**kw):
            return _gate_call(nv, L, name, **kw)
        req_args, req_x = (s.split() for s in _REQUIRED[name])
        nulls = [{a: None} for a in req_args] + [{"batch": {f: None}} for f in req_x]
        for dn in (a for a in names if a in ("d", "d1", "d2")):
            for k in _DIMS:
                assert call(dims={dn: {k: 0}}) == -1, (name, dn, k)
            assert call(dims={dn: {"V": 1}}) == -1, (name, dn, "V = 1")
            assert call(**{dn: None}) == -1, (name, dn, "NULL")
        for wn in (a for a in names if a.startswith("ws")):
            bn_ = "bytes" + wn[2:]
            assert call(**{wn: None}) == -1, (name, wn, "NULL")
            assert call(**{bn_: 8}) == -4, (name, bn_)
            assert call(**{bn_: 8, wn: _FAKE + 4}) == -4, (name, bn_, "too small and misaligned")
            for kw in nulls:
                assert call(**{bn_: 8}, **kw) == -4, (name, bn_, kw)
            assert call(**{wn: _FAKE + 4}) == -1, (name, wn, "misaligned")
        for kw in nulls:
            assert call(**kw) == -1, (name, kw)
    # ---- the entry points' own scalar tests
    call = lambda name, **kw: _gate_call(nv, L, name, **kw)      # noqa: E731
    assert call("xg_step_fwd", state=_FAKE + 4) == -1                                  # the in-place state needs 16-byte rows
    SAMPLE, REPLAY = nv.XG_ROLLOUT_SAMPLE, nv.XG_ROLLOUT_REPLAY
    assert call("xg_rollout", mode=SAMPLE, uniforms=None) == -1
    assert call("xg_rollout", mode=REPLAY, forced=None) == -1
    for temp in (0.0, -1.0, float("nan")):
        assert call("xg_rollout", mode=SAMPLE, temperature=temp) == -1, temp
        for name in ("xg_rollout_pair", "xg_rollout_pair_compact", "xg_rollout_pair_videos"):
            assert call(name, temperature=temp) == -1, (name, temp)
    for name, dn in (("xg_rollout", "d"), ("xg_rollout_pair", "d2"), ("xg_rollout_pair_compact", "d2"),
                     ("xg_rollout_pair_videos", "d2"), ("xg_rollout_bwd", "d")):
        assert call(name, dims={dn: {"T": 1}, "d1": {"T": 1}}) == -1, (name, "T < 2")
    for name in ("xg_rollout_pair", "xg_rollout_pair_compact"):
        for n in (0, -1, 2 * B, 2 * B + 1):                                            # (d2.B = 2 B here)
            assert call(name, n_sample=n) == -1, (name, n)
    assert call("xg_rollout_pair_compact", n_sample=B - 1) == -1                       # n_sample != d1->B
    assert call("xg_rollout_pair_videos", dims={"d2": {"B": 2 * B + 1}}) == -1         # d2->B != 2 * d1->B
    assert call("xg_rollout_pair_videos", ws1=_FAKE) == -1                             # ws1 == ws2
    assert call("xg_rollout_pair_videos", dims={"d1": {"R": 32}}) == -1                # d1 differs from d2 in R
    # xg_rollout_compact has no pointer of its own: what it refuses behind its two workspaces are dims that do not fit
    assert call("xg_rollout_compact", dims={"d1": {"R": 32}}) == -1
    assert call("xg_rollout_compact", dims={"d1": {"B": 2 * B + 1}}) == -1             # more rows than the rollout had
