"""CPU checks of the captioner's rollout over many pos_feats rows per video: the C ABI of include/xgate_control.h (exports,
version and constants through gcc, workspace sizes, every refusal without a GPU) and the Python surface -- the raises of
SAModel.sample_per_video and of the share_encoder keyword, and that the default path of control.py still calls sample on the
repeated inputs.  No compute on a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import paramgen as pg
from tests import util
from tests.util import ROOT

G = 4                                                           # XGCC_TEMPLATE_GROUP


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_control.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgcc_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgcc_rollout", "xgcc_version", "xgcc_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgcc_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_control.h":
            assert not re.search(r"xgcc_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_and_constants_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_control as ncc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_control.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGCC_VERSION, XG_VERSION, XGCC_TEMPLATE_GROUP);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, xver, grp = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = ncc.lib()
    assert ver == ncc.XGCC_VERSION == L.xgcc_version() == 1
    assert xver == nv.XG_VERSION == 206 and grp == ncc.XGCC_TEMPLATE_GROUP == G
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_control as ncc
    L = ncc.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    sizes = [L.xgcc_workspace_bytes(B(_mk(d)), S) for S in range(1, 10)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))      # grows with S
    for S in (0, -1):
        assert L.xgcc_workspace_bytes(B(_mk(d)), S) == 0
    assert L.xgcc_workspace_bytes(None, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1)):           # a rollout needs T >= 2
        assert L.xgcc_workspace_bytes(B(bad), 3) == 0
    assert L.xgcc_workspace_bytes(B(_mk(d, B=1 << 10)), 1 << 10) > 0           # 2^20 rows
    assert L.xgcc_workspace_bytes(B(_mk(d, B=1 << 10)), (1 << 10) + 1) == 0    # ... and beyond
    assert L.xgcc_workspace_bytes(B(_mk(d, B=1 << 20)), 2) == 0
    # the real sizes: 64 videos under 8 templates each against the workspace of the 512-row batch
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=64))
    shared = L.xgcc_workspace_bytes(B(_mk(c1)), 8)
    repeated = nv.lib().xg_workspace_bytes(B(_mk(c1, B=64 * 8)))
    print("configs[1] dims, B = 64, S = 8: xgcc_workspace_bytes %d (%.1f MB), xg_workspace_bytes of 512 rows %d (%.1f MB)"
          % (shared, shared / 2 ** 20, repeated, repeated / 2 ** 20))
    assert 0 < shared < repeated
    # the row part holds no (M,K,R) or (M,K,A) tensor: 8 more rows per video cost far less than 8 more copies of v2a(V) and V
    per_row = (L.xgcc_workspace_bytes(B(_mk(c1)), 16) - shared) / (64 * 8)
    assert per_row < 4 * c1.K * c1.A


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_control as ncc
    L = ncc.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgcc_workspace_bytes(B(dims), 3)
    fake = 256
    P = nv.XgParams(*([fake] * len(nv.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40
    GREEDY, SAMPLE, REPLAY = nv.XG_ROLLOUT_GREEDY, nv.XG_ROLLOUT_SAMPLE, nv.XG_ROLLOUT_REPLAY

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

    def call(dm=dims, S=3, p=P, b=bn, x=None, r=None, mode=GREEDY, u=None, temp=1.0, outs=None, ws=fake, nbytes=big):
        o = [fake] * 3 if outs is None else outs       # seq, seq_logp, n_steps
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgcc_rollout(None, B(dm), S, None if p is None else B(p), None if b is None else B(b), None if x is False else B(x),
                              None if r is False else B(r), mode, u, temp, o[0], o[1], o[2], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(S=4, nbytes=need) == -4                                       # the workspace of S = 3 does not serve S = 4
    assert call(mode=SAMPLE, u=fake, temp=0.7, nbytes=8) == -4
    # XG_EINVAL
    assert call(S=0) == -1 and call(S=-2) == -1
    assert call(dm=_mk(d, B=0)) == -1 and call(dm=_mk(d, L=0)) == -1 and call(dm=_mk(d, B=1 << 10), S=(1 << 10) + 1) == -1
    assert call(r=run(train=1)) == -1 and call(r=run(save=1)) == -1
    assert call(r=run(gemm_mode=1)) == -1 and call(r=run(gemm_mode=3)) == -1
    assert call(mode=REPLAY) == -1 and call(mode=REPLAY, u=fake) == -1 and call(mode=17) == -1
    assert call(mode=SAMPLE) == -1                                            # no uniforms
    assert call(mode=SAMPLE, u=fake, temp=0.0) == -1 and call(mode=SAMPLE, u=fake, temp=-1.0) == -1
    assert call(mode=SAMPLE, u=fake, temp=float("nan")) == -1
    assert call(b=None) == -1                                                 # eval mode reads the running statistics
    for i in range(4):
        st = [fake] * 4
        st[i] = None
        assert call(b=nv.XgBnState(*st)) == -1, i
    assert call(ws=fake + 16) == -1 and call(ws=None) == -1                   # the workspace is 256-byte aligned
    assert call(p=None) == -1 and call(x=False) == -1 and call(r=False) == -1
    for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"):
        assert call(x=batch(**{k: None})) == -1, k
    for i in range(3):
        outs = [fake] * 3
        outs[i] = None
        assert call(outs=outs) == -1, i


# ---- the Python surface
def test_sample_per_video_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    with pytest.raises(NotImplementedError):                # train mode
        m.sample_per_video(*f, pos)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.sample_per_video(*f, pos)
    with pytest.raises(NotImplementedError):
        m.sample_per_video(*f, pos, {"beam_size": 2})
    with pytest.raises(NotImplementedError):
        m.sample_per_video(*f, pos, {"forced_tokens": torch.zeros(d.B * S, d.L, dtype=torch.int64)})
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.sample_per_video(*f, bad)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.sample_per_video(*f, pos)


class _StubPos:
    """sample_forced / sample_templates / beam_templates of a POS model, as far as control.py reads them."""

    def __init__(self, B, S, L, R):
        self.B, self.S, self.L, self.R = B, S, L, R
        self.pos_feats = torch.arange(B * S * R, dtype=torch.float32).reshape(B * S, R)

    def sample_forced(self, fr, fo, fm, templates, collect_states=False, trim=False):
        return torch.full((self.B, self.S, self.L), -0.5), None, None, self.pos_feats

    def sample_templates(self, fr, fo, fm, S, **kw):
        return torch.zeros(self.B, S, self.L, dtype=torch.int64), torch.full((self.B, S, self.L), -0.5), None, None, self.pos_feats

    def beam_templates(self, fr, fo, fm, beam_size=5, suppress_tag=1, trim=False):
        return torch.zeros(self.B, self.S, self.L, dtype=torch.int64), None, torch.zeros(self.B, self.S), None


class _StubCap:
    def __init__(self, n):
        self.n, self.calls = n, []

    def sample(self, fr, fo, fm, pos, opt={}):
        self.calls.append(("sample", fr, fo, fm, pos, opt))
        M = fr.shape[0]
        return torch.arange(M * self.n).reshape(M, self.n), torch.zeros(M, self.n)

    def sample_per_video(self, fr, fo, fm, pos, opt={}):
        self.calls.append(("sample_per_video", fr, fo, fm, pos, opt))
        B, S = pos.shape[:2]
        return torch.arange(B * S * self.n).reshape(B, S, self.n), torch.zeros(B, S, self.n)


def test_share_encoder_keyword_with_stub_models():
    from controllable_xgating_amd import caption_beam, caption_sampled, caption_with_templates
    B, S, L, R, K, n = 3, 4, 5, 6, 2, 5
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm = _StubPos(B, S, L, R)
    tm = torch.zeros(B, S, L, dtype=torch.int64)
    opt = {"sample_max": 1}
    chains = {"with_templates": lambda cap, **kw: caption_with_templates(pm, cap, fr, fo, fm, tm, opt, **kw),
              "sampled": lambda cap, **kw: caption_sampled(pm, cap, fr, fo, fm, S, opt=opt, **kw),
              "beam": lambda cap, **kw: caption_beam(pm, cap, fr, fo, fm, beam_size=S, opt=opt, **kw)}
    for name, chain in chains.items():
        for kw in ({}, {"share_encoder": False}):       # the default: sample on the inputs repeated per template, as before
            cap = _StubCap(n)
            out = chain(cap, **kw)
            (kind, a, b, c, pos, o), = cap.calls
            assert kind == "sample" and o is opt, name
            assert torch.equal(a, fr.repeat_interleave(S, 0)) and torch.equal(b, fo.repeat_interleave(S, 0)), name
            assert torch.equal(c, fm.repeat_interleave(S, 0)) and pos is pm.pos_feats, name
            assert out[0].shape == (B, S, n) and torch.equal(out[0], torch.arange(B * S * n).reshape(B, S, n)), name
        cap = _StubCap(n)
        out = chain(cap, share_encoder=True)
        (kind, a, b, c, pos, o), = cap.calls
        assert kind == "sample_per_video" and a is fr and b is fo and c is fm and o is opt, name
        assert pos.shape == (B, S, R) and torch.equal(pos.reshape(B * S, R), pm.pos_feats), name
        assert out[0].shape == (B, S, n) and out[1].shape == (B, S, n), name
        cap = _StubCap(n)
        with pytest.raises(NotImplementedError):
            {"with_templates": lambda: caption_with_templates(pm, cap, fr, fo, fm, tm, {"beam_size": 3}, share_encoder=True),
             "sampled": lambda: caption_sampled(pm, cap, fr, fo, fm, S, opt={"beam_size": 3}, share_encoder=True),
             "beam": lambda: caption_beam(pm, cap, fr, fo, fm, beam_size=S, opt={"beam_size": 3}, share_encoder=True)}[name]()
        assert not cap.calls                            # refused before either model ran
