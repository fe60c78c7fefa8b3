"""CPU checks of the captioner's beam search under S POS templates per video: the C ABI of include/xgate_beam_control.h (exports,
version through gcc, workspace sizes, every refusal without a GPU) and the Python surface -- the raises of
SAModel.beam_captions_per_video, what control.beam_captions_with_templates hands over, and that share_encoder=True with a beam
still raises.  No compute on a GPU."""
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


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_beam_control.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgbc_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgbc_beam_search", "xgbc_version", "xgbc_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgbc_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_beam_control.h":
            assert not re.search(r"xgbc_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_control as nbc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_beam_control.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGBC_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = nbc.lib()
    assert ver == nbc.XGBC_VERSION == L.xgbc_version() == 1 and xver == nv.XG_VERSION
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native_beam as nb
    from controllable_xgating_amd import _native_beam_control as nbc
    L = nbc.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    size = lambda S, W, dm=None: L.xgbc_workspace_bytes(B(_mk(d) if dm is None else dm), S, W)      # noqa: E731
    assert size(1, 1) > 0
    assert all(size(S, 3) < size(S + 1, 3) for S in range(1, 9)) and all(size(3, W) < size(3, W + 1) for W in range(1, 8))
    for S, W in ((0, 3), (-1, 3), (3, 0), (3, -1), (3, 9), (3, 64)):
        assert size(S, W) == 0, (S, W)
    assert L.xgbc_workspace_bytes(None, 3, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1)):           # a search needs T >= 2
        assert size(3, 3, bad) == 0
    assert size(3, 6, _mk(d, V=5)) == 0 and size(3, 5, _mk(d, V=5)) > 0          # W > V
    assert size(1 << 7, 8, _mk(d, B=1 << 10)) > 0                               # 2^20 rows
    assert size((1 << 7) + 1, 8, _mk(d, B=1 << 10)) == 0                        # ... and beyond
    assert size(1 << 8, 8, _mk(d, B=1 << 10)) == 0 and size(2, 1, _mk(d, B=1 << 20)) == 0
    # the real sizes: 64 videos under 8 templates, 5 beams each, against the plain search's workspace for the 512 repeated videos
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=64))
    S, W = 8, 5
    M = 64 * S * W
    shared = size(S, W, _mk(c1))
    repeated = nb.lib().xgcb_workspace_bytes(B(_mk(c1, B=64 * S)), W)
    print("configs[1] dims, B = 64, S = 8, W = 5: xgbc_workspace_bytes %d (%.1f MB), xgcb_workspace_bytes at B = 512 %d (%.1f MB)"
          % (shared, shared / 2 ** 20, repeated, repeated / 2 ** 20))
    assert 0 < shared and repeated - shared >= M * c1.K * (c1.R + c1.A) * 4
    for s in (1, 4):
        print("S = %d: %.1f MB" % (s, size(s, W, _mk(c1)) / 2 ** 20))


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_control as nbc
    L = nbc.lib()
    d = pg.make_dims(**util.CFG["mid"])                            # V = 500
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgbc_workspace_bytes(B(dims), 2, 3)
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

    def call(dm=dims, S=2, W=3, sup=1, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 4 if outs is None else outs       # seq, seq_logp, score, trace
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgbc_beam_search(None, B(dm), S, W, sup, None if p is None else B(p), None if b is None else B(b),
                                  None if x is False else B(x), None if r is False else B(r), o[0], o[1], o[2], o[3], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(W=4, nbytes=need) == -4 and call(S=3, nbytes=need) == -4         # the workspace of (2, 3) serves neither
    assert call(S=1, W=1, nbytes=8) == -4 and call(W=8, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=-7, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=499, nbytes=8) == -4
    assert call(outs=[fake, fake, fake, None], nbytes=8) == -4                # trace may be NULL: the next check decides
    # XG_EINVAL: what the plain search refuses ...
    for W in (0, -1, 9, 64):
        assert call(W=W) == -1, W
    v5 = _mk(d, V=5)
    assert call(dm=v5, W=5, nbytes=8) == -4 and call(dm=v5, W=6) == -1        # W > V
    assert call(sup=500) == -1 and call(sup=1 << 20) == -1 and call(dm=v5, sup=5) == -1
    assert call(dm=_mk(d, B=0)) == -1 and call(dm=_mk(d, L=0)) == -1
    assert call(r=run(train=1)) == -1 and call(r=run(save=1)) == -1
    assert call(r=run(gemm_mode=1)) == -1 and call(r=run(gemm_mode=3)) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(x=False) == -1 and call(r=False) == -1 and call(ws=None) == -1
    assert call(ws=fake + 16) == -1                                           # the workspace is 256-byte aligned
    for i in range(4):
        st = [fake] * 4
        st[i] = None
        assert call(b=nv.XgBnState(*st)) == -1, i
    for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"):
        assert call(x=batch(**{k: None})) == -1, k
    for i in range(3):
        outs = [fake] * 4
        outs[i] = None
        assert call(outs=outs) == -1, i
    # ... S < 1, and more than 2^20 rows
    assert call(S=0) == -1 and call(S=-2) == -1
    k10 = _mk(d, B=1 << 10)
    assert call(dm=k10, S=1 << 7, W=8, nbytes=8) == -4 and call(dm=k10, S=(1 << 7) + 1, W=8) == -1


# ---- the Python surface
def test_beam_captions_per_video_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    with pytest.raises(NotImplementedError):                # train mode
        m.beam_captions_per_video(*f, pos, beam_size=3)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.beam_captions_per_video(*f, pos, beam_size=3)
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.beam_captions_per_video(*f, bad, beam_size=3)
    for W in (0, 9, d.V + 1):
        with pytest.raises(ValueError):
            m.beam_captions_per_video(*f, pos, beam_size=W)
    with pytest.raises(ValueError):
        m.beam_captions_per_video(*f, pos, beam_size=3, suppress_token=d.V)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.beam_captions_per_video(*f, pos, beam_size=3)


class _StubPos:
    def __init__(self, B, S, L, R):
        self.B, self.S, self.L, self.R = B, S, L, R
        self.pos_feats = torch.arange(B * S * R, dtype=torch.float32).reshape(B * S, R)
        self.calls = []

    def sample_forced(self, fr, fo, fm, templates, collect_states=False, trim=False):
        self.calls.append((fr, fo, fm, templates, collect_states, trim))
        return torch.full((self.B, self.S, self.L), -0.5), None, None, self.pos_feats


class _StubCap:
    def __init__(self, L):
        self.L, self.calls = L, []

    def beam_captions_per_video(self, fr, fo, fm, pos, beam_size=5, suppress_token=1, return_trace=False):
        self.calls.append((fr, fo, fm, pos, beam_size, suppress_token, return_trace))
        B, S = pos.shape[:2]
        n = B * S * beam_size * self.L
        return torch.arange(n).reshape(B, S, beam_size, self.L), torch.zeros(B, S, beam_size, self.L), torch.ones(B, S, beam_size)

    def sample(self, *a, **k):
        raise AssertionError("the repeated path ran")

    beam_captions = sample_per_video = sample


def test_beam_captions_with_templates_hands_the_videos_over_once():
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import beam_captions_with_templates
    assert "beam_captions_with_templates" in pkg.__all__
    B, S, L, R, K, W = 3, 4, 5, 6, 2, 3
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, S, L, R), _StubCap(L)
    tm = torch.zeros(B, S, L, dtype=torch.int64)
    seq, lp, score, tscore = beam_captions_with_templates(pm, cap, fr, fo, fm, tm, beam_size=W, suppress_token=-1)
    (a, b, c, t, collect, trim), = pm.calls
    assert a is fr and b is fo and c is fm and t is tm and collect is False and trim is False
    (a, b, c, pos, w, sup, tr), = cap.calls
    assert a is fr and b is fo and c is fm                                    # un-repeated: the very tensors
    assert pos.shape == (B, S, R) and torch.equal(pos.reshape(B * S, R), pm.pos_feats)
    assert (w, sup, tr) == (W, -1, False)
    assert seq.shape == (B, S, W, L) and lp.shape == seq.shape and score.shape == (B, S, W)
    assert tscore.shape == (B, S) and torch.allclose(tscore, torch.full((B, S), -0.5 * L))
    cap = _StubCap(L)
    beam_captions_with_templates(pm, cap, fr, fo, fm, tm)
    assert cap.calls[0][4:6] == (5, 1)                                        # the defaults of beam_captions


def test_share_encoder_with_a_beam_still_raises():
    from controllable_xgating_amd import caption_beam, caption_sampled, caption_with_templates
    B, S, L, R, K = 3, 4, 5, 6, 2
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, S, L, R), _StubCap(L)
    tm = torch.zeros(B, S, L, dtype=torch.int64)
    for chain in (lambda: caption_with_templates(pm, cap, fr, fo, fm, tm, {"beam_size": 5}, share_encoder=True),
                  lambda: caption_sampled(pm, cap, fr, fo, fm, S, opt={"beam_size": 5}, share_encoder=True),
                  lambda: caption_beam(pm, cap, fr, fo, fm, beam_size=S, opt={"beam_size": 5}, share_encoder=True)):
        with pytest.raises(NotImplementedError, match="beam_captions_with_templates"):
            chain()
    assert not pm.calls and not cap.calls                                     # refused before either model ran
    m = util.make_model(pg.make_dims(**util.CFG["tiny"]), device="cpu", train=False)
    with pytest.raises(NotImplementedError):
        m.sample_per_video(fr, fo, fm, torch.zeros(B, S, 24), {"beam_size": 2})
