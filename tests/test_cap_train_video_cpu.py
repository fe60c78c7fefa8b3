"""CPU checks of teacher-forced training on Q captions per video (include/xgate_train_video.h): the composed oracle
(tests/cap_train_video_oracle.py) against forward_xe on the repeated batch, the preconditions of the GPU cases, the C ABI -- exports,
version, workspace sizes, every refusal in the documented order without a GPU --, data.collate_per_video and the raises of
SAModel.xe_loss_per_video.  No compute on a GPU."""
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
from tests import cap_train_video_oracle as tvo
from tests import util
from tests.util import ROOT, ZERO_GRAD_PARAMS, grad_misses


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the oracle helper
@pytest.mark.parametrize("name", ["tiny", "odd", "one_q5", "mid"])
def test_composed_oracle_equals_forward_xe_on_the_repeated_batch(name):
    d, Q, _, _, _ = tvo.case_inputs(name)
    a, b = tvo.case_reference(name), tvo.repeated_reference(name)
    for k in ("loss", "lm", "cls"):
        assert abs(a[k] - b[k]) <= 1e-6, (k, a[k], b[k])
    bad = grad_misses(a["grads"], b["grads"], skip=ZERO_GRAD_PARAMS)
    assert not bad, bad
    n, nm = d.B * d.K, d.B * Q * d.K
    fa, fb = n / max(n - 1, 1), nm / max(nm - 1, 1)          # the two unbiased factors
    for mod in ("rgb", "opfl"):
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(a["running"][pre + "running_mean"].numpy(), b["running"][pre + "running_mean"].numpy(), atol=1e-7)
        va, vb = a["running"][pre + "running_var"].numpy(), b["running"][pre + "running_var"].numpy()
        # running_var = 0.9 + 0.1 * biased batch variance * factor: the batch variance is the same, the factors are not
        np.testing.assert_allclose((va - 0.9) / fa, (vb - 0.9) / fb, rtol=1e-5, atol=1e-7)
        if Q > 1 and n > 1:
            assert np.abs(va - vb).max() > 0


def test_cases_hold_what_they_name():
    for name, (cfg, B, Q, _) in tvo.CASES.items():
        d, Q_, P, xv, xr = tvo.case_inputs(name)
        M, T = B * Q, d.L + 1
        assert Q_ == Q and d.B == B and xv["feats_rgb"].shape[0] == B and xr["seq"].shape == (M, T) and xr["pos_feats"].shape == (M, d.R)
        assert (xr["seq"][:, 0] == 0).all() and (xr["seq_mask"][:, 0] == 1).all()
    d, Q, _, xv, xr = tvo.case_inputs("tiny")
    assert (xv["feat_mask"] == 0).any()                                                       # ragged feat_mask
    lens = xr["seq_mask"].sum(1).reshape(d.B, Q)
    assert (lens.max(1) > lens.min(1)).all()                                                  # ragged between the captions of one video
    b, q = tvo.PADDED_ROW["tiny"]
    assert xr["seq_mask"][b * Q + q].sum() == 1 and (xr["seq"][b * Q + q] == 0).all()         # all padding behind BOS
    d, Q, _, _, xr = tvo.case_inputs("mid")
    b = tvo.IDENTICAL_VIDEO["mid"]
    for a in xr.values():
        assert (a[b * Q:(b + 1) * Q] == a[b * Q]).all()
    assert not (xr["seq"][0] == xr["seq"][1]).all()


def test_cases_reach_the_branches_they_name():
    src = open(os.path.join(ROOT, "controllable_xgating_amd", "csrc", "xg_kernels.h")).read()
    assert int(re.search(r"XGK_ATTN_BWD_GROUP\s*=\s*(\d+)", src).group(1)) == tvo.GROUP
    c = {k: util.CFG[v[0]] for k, v in tvo.CASES.items()}
    q = {k: v[2] for k, v in tvo.CASES.items()}
    G = tvo.GROUP
    # the per-step attention backward: group form (mid, c1; partial groups at Q = 5, 3, 1; whole ones at Q = 4), rows form (odd)
    assert tvo.attn_bwd_group_form(c["mid"]) and tvo.attn_bwd_group_form(c["c1"]) and tvo.attn_bwd_group_form(c["one_q5"])
    assert not tvo.attn_bwd_group_form(c["odd"]) and c["odd"]["R"] % 8 and not tvo.packed(c["odd"])      # ... and the generic step
    assert tvo.attn_bwd_group_form(c["tiny"]) and not tvo.packed(c["tiny"]) and c["tiny"]["R"] % 8 == 0  # the LDS-staged step
    assert tvo.packed(c["mid"]) and tvo.packed(c["c1"])
    assert q["mid"] == G + 1 and q["mid_q3"] < G and q["c1"] == G and q["one_q5"] == G + 1 and q["one_q1"] == 1
    assert c["c1"]["A"] > 512 and c["c1"]["A"] % 512 == 0 and c["mid"]["A"] < 512                        # several column parts / one, partial
    assert c["one_q5"]["K"] == 1 and c["one_q5"]["L"] + 1 == 2
    # the group kernel holds 32 frames of its q column and 8 pieces of V per lane up front: c5 goes round both loops a second time
    pieces = lambda d: -(-d["K"] // 8) * -(-d["R"] // 256)      # noqa: E731  (rows of wave 0 x 256-float chunks of a row)
    assert tvo.attn_bwd_group_form(c["c5"]) and c["c5"]["K"] > 32 and pieces(c["c5"]) > 8
    assert all(c[k]["K"] <= 32 and pieces(c[k]) <= 8 for k in ("tiny", "mid", "c1", "one_q5"))
    # the post-loop pass (one launcher branch): frame parts of one frame (mid_q224), of several with a shorter last one (c1: 7, 7,
    # 7, 5; mid: 2, 2, 2, 2, 1), one part with every frame (Q = 1); chunks of 16 (step, row) pairs, the last one partial, one or many
    assert tvo.post_frame_parts(c["c1"], q["c1"])[:2] == (4, 7) and c["c1"]["K"] % 7
    assert tvo.post_frame_parts(c["mid"], q["mid"])[:2] == (5, 2) and c["mid"]["K"] % 2
    assert tvo.post_frame_parts(c["mid_q224"], q["mid_q224"]) == (9, 1, 112)
    assert tvo.post_frame_parts(c["mid_q1"], 1)[:2] == (1, 9) and tvo.post_frame_parts(c["one_q5"], 5) == (1, 1, 1)
    assert ((c["mid"]["L"] + 1) * q["mid"]) % 16 and ((c["c1"]["L"] + 1) * q["c1"]) % 16 and (c["one_q1"]["L"] + 1) * q["one_q1"] < 16
    assert (c["c1"]["R"], c["c1"]["A"], c["c1"]["K"], c["c1"]["V"]) == (512, 1536, 26, 20000)


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_train_video.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgtv_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgtv_version", "xgtv_video_grads", "xgtv_workspace_bytes", "xgtv_xe_loss_bwd", "xgtv_xe_loss_fwd"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgtv_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_train_video.h":
            assert not re.search(r"xgtv_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc_and_xg_abi_unchanged(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_train_video as ntv
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_train_video.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(XgDims), sizeof(XgParams), sizeof(XgBnState), sizeof(XgBatch), '
                   'sizeof(XgRun), XGTV_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, sb, sx, sr, ver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ver == ntv.XGTV_VERSION == ntv.lib().xgtv_version() == 1
    assert xver == nv.XG_VERSION == 206
    assert (sd, sp, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgParams, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_train_video as ntv
    L = ntv.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    for Q in (0, -1):
        assert L.xgtv_workspace_bytes(B(_mk(d)), Q) == 0
    assert L.xgtv_workspace_bytes(None, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1), _mk(d, K=0)):
        assert L.xgtv_workspace_bytes(B(bad), 3) == 0
    assert L.xgtv_workspace_bytes(B(_mk(d, B=1 << 10)), (1 << 10) + 1) == 0    # beyond 2^20 rows
    # the real layer sizes, B = 32 videos
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=32))
    T = c1.L + 1
    w = {Q: L.xgtv_workspace_bytes(B(_mk(c1)), Q) for Q in (1, 2, 3, 4, 6, 8)}
    assert all(v > 0 for v in w.values())
    whole = nv.lib().xg_workspace_bytes(B(_mk(c1, B=32 * 4)))
    print("configs[1] dims, B = 32: xgtv_workspace_bytes Q = 4 %d (%.1f MB), xg_workspace_bytes of the 128-row batch %d (%.1f MB)"
          % (w[4], w[4] / 2 ** 20, whole, whole / 2 ** 20))
    assert w[4] < whole
    assert w[4] < nv.lib().xg_workspace_bytes_mode(B(_mk(c1, B=32 * 4)), 0)                   # ... and without the bf16 mirror region
    # linear in Q: equal steps between even Q (every block of the row part is then a multiple of its 256-byte alignment), and
    # within the two (T M)-float blocks' padding of 128 bytes each at odd Q
    step = w[4] - w[2]
    assert step > 0 and w[6] - w[4] == step and w[8] - w[6] == step
    assert w[1] < w[2] < w[3] < w[4] and abs(2 * (w[3] - w[2]) - step) <= 512 and abs(2 * (w[2] - w[1]) - step) <= 512
    # the per-row cost holds no K R or K A term: from two frame counts, a further frame costs a row its alpha and de of the T steps only
    per_row = {}
    for K in (26, 58):
        dk = _mk(c1, K=K)
        per_row[K] = (L.xgtv_workspace_bytes(B(dk), 8) - L.xgtv_workspace_bytes(B(dk), 4)) / (4 * 32)
    per_frame = (per_row[58] - per_row[26]) / 32
    print("bytes per further row %.0f (K = 26), %.0f (K = 58): %.1f per frame and row (2 T floats = %d; one row of V alone %d)"
          % (per_row[26], per_row[58], per_frame, 8 * T, 4 * c1.R))
    assert per_frame == 8 * T
    assert per_frame < 4 * c1.R and per_frame < 4 * c1.A


def test_bad_arguments_return_error_codes_in_the_documented_order_without_a_gpu(built):
    """As xgsc_score_captions (docs/CAPTION_SCORE.md): bad dims (Q among them) or a NULL workspace -1, a workspace that is too small
    -4 -- whatever else is wrong with the call --, a misaligned workspace -1, and only then the entry point's own pointer and run
    tests -1.  Every pointer is a fake that is never dereferenced: nothing is enqueued."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_train_video as ntv
    L = ntv.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgtv_workspace_bytes(B(dims), 3)
    fake = 0x7F0000000000
    P = nv.XgParams(*([fake] * len(nv.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def batch(**kw):
        v = dict(feats_rgb=fake, feats_opfl=fake, feat_mask=fake, pos_feats=fake, seq=fake, seq_mask=fake)
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

    def fwd(dm=dims, Q=3, p=P, b=bn, x=None, r=None, out=fake, ws=fake, nbytes=big, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgtv_xe_loss_fwd(None, ref(dm), Q, ref(p), ref(b), ref(x), None, None, 0.0, ref(r), ws, nbytes, out)

    def bwd(dm=dims, Q=3, p=P, g=P, x=None, r=None, out=fake, ws=fake, nbytes=big, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgtv_xe_loss_bwd(None, ref(dm), Q, ref(p), ref(g), ref(x), None, None, 0.0, out, ref(r), ws, nbytes)

    def vg(dm=dims, Q=3, p=P, out=fake, ws=fake, nbytes=big, **_):
        return L.xgtv_video_grads(None, ref(dm), Q, ref(p), ws, nbytes, out, out)

    first = (dict(Q=0), dict(Q=-2), dict(dm=None), dict(dm=_mk(d, B=0)), dict(dm=_mk(d, L=0)), dict(dm=_mk(d, V=1)),
             dict(dm=_mk(d, B=1 << 10), Q=(1 << 10) + 1), dict(ws=None))
    later = [dict(p=None), dict(x=False), dict(r=False), dict(r=run(gemm_mode=1)), dict(r=run(gemm_mode=3)), dict(ws=fake + 16), dict(out=None)]
    later += [dict(x=batch(**{k: None})) for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats", "seq", "seq_mask")]
    for call, own in ((fwd, [dict(r=run(train=0), b=None), dict(r=run(train=0), b=nv.XgBnState(fake, None, fake, fake))]),
                      (bwd, [dict(g=None)]), (vg, [])):
        skip = ("x", "r") if call is vg else ()
        mine = [kw for kw in later + own if not any(k in kw for k in skip)]
        for kw in first:                              # 1. -1, also with a workspace that is too small
            assert call(**kw) == -1 and call(**dict(kw, nbytes=8)) == -1, (call.__name__, kw)
        assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4            # 2. too small: -4, whatever else is wrong behind it
        assert call(Q=4, nbytes=need) == -4                                    # the workspace of Q = 3 does not serve Q = 4
        for kw in mine:
            assert call(**dict(kw, nbytes=8)) == -4, (call.__name__, kw)
        for kw in mine:                               # 3. everything else: -1
            assert call(**kw) == -1, (call.__name__, kw)
            assert call(**dict(kw, nbytes=need)) == -1, (call.__name__, kw)
    assert fwd(r=run(train=0), b=None, nbytes=8) == -4


# ---- data.collate_per_video
def test_collate_per_video_shapes_and_contents():
    from controllable_xgating_amd.data import collate, collate_per_video
    g = torch.Generator().manual_seed(3)
    B, Q, K, F1, F2, R = 3, 2, 4, 5, 3, 6
    lens = [3, 1, 2, 5, 4, 4]
    items = []
    for b in range(B):
        f1, f2 = torch.rand(K, F1, generator=g), torch.rand(K, F2, generator=g)
        fm = torch.ones(1, K)
        fm[0, K - b:] = 0
        for q in range(Q):
            n = lens[b * Q + q]
            items.append(dict(id="v%d" % b, cap=[2 + (b * Q + q + j) % 7 for j in range(n)], cap_class=[(b + q + j) % 4 for j in range(n + 1)],
                              class_mask=[1.0] * n, feat1=f1, feat2=f2, feat_mask=fm, pos_feat=torch.rand(R, generator=g)))
    caps, cmask, ccls, clmask, feats1, feats2, fmask, pos = collate_per_video(items, Q)
    T = max(lens) + 1
    assert caps.shape == cmask.shape == ccls.shape == clmask.shape == (B, Q, T) and caps.dtype == ccls.dtype == torch.int64
    assert feats1.shape == (B, K, F1) and feats2.shape == (B, K, F2) and fmask.shape == (B, K) and pos.shape == (B, Q, R)
    for b in range(B):
        assert torch.equal(feats1[b], items[b * Q]["feat1"]) and torch.equal(feats2[b], items[b * Q]["feat2"])
        assert torch.equal(fmask[b], items[b * Q]["feat_mask"][0])
        for q in range(Q):
            it = items[b * Q + q]
            one = collate([it])                        # the row fields are collate's, zero-padded to the batch's longest caption
            n = len(it["cap"])
            for got, want in zip((caps, cmask, ccls, clmask), one[:4]):
                assert torch.equal(got[b, q, :n + 1], want[0]) and (got[b, q, n + 1:] == 0).all()
            assert caps[b, q, 0] == 0 and caps[b, q, 1:n + 1].tolist() == it["cap"] and cmask[b, q].sum() == n + 1
            assert torch.equal(pos[b, q], it["pos_feat"])
    for bad_q in (0, 4, -1):
        with pytest.raises(ValueError):
            collate_per_video(items, bad_q)
    with pytest.raises(ValueError):
        collate_per_video(items[1:] + items[:1], Q)   # rows of two videos in one group
    with pytest.raises(ValueError):
        collate_per_video([], Q)


# ---- the Python surface
def test_xe_loss_per_video_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    Q, T = 3, d.L + 1
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, Q, d.R)
    seq = torch.zeros(d.B, Q, T, dtype=torch.int64)
    mask = torch.ones(d.B, Q, T)
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.xe_loss_per_video(*f, pos, seq, mask)
    for bad in (pos.reshape(d.B * Q, d.R), pos[1:], pos[:, :, 1:], pos[:, :2], pos.unsqueeze(0)):
        with pytest.raises(ValueError):
            m.xe_loss_per_video(*f, bad, seq, mask)
    for bad in (seq.reshape(d.B * Q, T), seq[1:], seq[:, :2], seq[:, :, :1], seq.float(), seq[:, :0]):
        with pytest.raises(ValueError):
            m.xe_loss_per_video(*f, pos, bad, mask)
    for bad in (mask.reshape(d.B * Q, T), mask[:, :, 1:], mask[:, :2]):
        with pytest.raises(ValueError):
            m.xe_loss_per_video(*f, pos, seq, bad)
    for bad in ((f[0][1:], f[1], f[2]), (f[0], f[1][:, 1:], f[2]), (f[0], f[1], f[2][:, 1:]), (f[0][:, :, 1:], f[1], f[2]),
                (f[0].reshape(d.B * d.K, -1), f[1], f[2])):
        with pytest.raises(ValueError):
            m.xe_loss_per_video(*bad, pos, seq, mask)
    with pytest.raises(ValueError):
        m.xe_loss_per_video(*f, pos, seq, mask, cap_classes=seq[:, :2], weight_class=0.5)
    with pytest.raises(ValueError):
        m.xe_loss_per_video(*f, pos, seq, mask, cap_classes=seq, class_mask=mask[:, :, 0], weight_class=0.5)
    m.ss_prob = 0.25
    with pytest.raises(NotImplementedError):                # scheduled sampling
        m.xe_loss_per_video(*f, pos, seq, mask)
    m.eval()                                                # (eval mode never samples: only the device is missing)
    with pytest.raises(NotImplementedError):
        m.xe_loss_per_video(*f, pos, seq, mask)
    m.ss_prob = 0.0
    m.train()
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.xe_loss_per_video(*f, pos, seq, mask)
    m.precision = "bf16x3"
    with pytest.raises(NotImplementedError):
        m.xe_loss_per_video(*f, pos, seq, mask)
    assert hasattr(type(m), "xe_loss_per_video")
