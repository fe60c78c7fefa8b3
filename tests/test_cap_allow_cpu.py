"""CPU checks of the captioner's beam search whose words must follow a POS template: the C ABI of include/xgate_beam_allow.h
(exports, version through gcc, workspace sizes, every refusal without a GPU), the Python surface (every raise of
SAModel.beam_captions_allowed, data.word_category_table, control.allow_masks, control.template_adherence, what
control.beam_captions_following_templates hands over), the oracle helper tests/cap_allow_oracle.py against itself, and the
PRECONDITIONS of the cases tests/test_gpu_cap_allow.py runs, on the float64 oracle alone.  No compute on a GPU.

Pinned groups (float64 selection margin >= 1e-3) of the cases whose seed and gain were chosen here, counted by
test_preconditions_of_the_gpu_cases: tiny_s3w3 (input seed 1, gain 32, table seed 5) 15 of 15, mid_s4w5 (seed 2, gain 128, table
seed 7) 44 of 48, the short-row case (tiny, S 3, W 3, input seed 4, gain 32, table seed 5, PAIR at position 0) 15 of 15."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_allow_oracle as cao
from tests import cap_beam_oracle as cbo
from tests import util
from tests.util import ROOT

ANY = cao.ANY


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_beam_allow.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgba_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgba_beam_search", "xgba_version", "xgba_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgba_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_beam_allow.h":
            assert not re.search(r"xgba_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_allow as nba
    from controllable_xgating_amd import _native_beam_control as nbc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_beam_allow.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGBA_VERSION, XGBC_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, cver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                      text=True).stdout.split())
    L = nba.lib()
    assert ver == nba.XGBA_VERSION == L.xgba_version() == 1
    assert cver == nbc.XGBC_VERSION and xver == nv.XG_VERSION                   # the other versions did not move
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    """0 wherever the unconstrained search's size is 0, at least that size otherwise."""
    from controllable_xgating_amd import _native_beam_allow as nba
    from controllable_xgating_amd import _native_beam_control as nbc
    La, Lc = nba.lib(), nbc.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=64))
    k10 = _mk(d, B=1 << 10)
    dims = [(_mk(d), S, W) for S in (-1, 0, 1, 2, 3, 8) for W in (-1, 0, 1, 3, 5, 8, 9, 64)]
    dims += [(bad, 3, 3) for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1))]
    dims += [(_mk(d, V=5), 3, 6), (_mk(d, V=5), 3, 5), (k10, 1 << 7, 8), (k10, (1 << 7) + 1, 8), (_mk(d, B=1 << 20), 2, 1)]
    dims += [(_mk(c1), S, 5) for S in (1, 4, 8)]
    zeros = 0
    for dm, S, W in dims:
        a, c = La.xgba_workspace_bytes(B(dm), S, W), Lc.xgbc_workspace_bytes(B(dm), S, W)
        assert (a == 0) == (c == 0) and a >= c, (S, W, a, c)
        zeros += a == 0
    assert 0 < zeros < len(dims)
    assert La.xgba_workspace_bytes(None, 3, 3) == 0
    assert all(La.xgba_workspace_bytes(B(_mk(d)), S, 3) < La.xgba_workspace_bytes(B(_mk(d)), S + 1, 3) for S in range(1, 9))


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_allow as nba
    L = nba.lib()
    d = pg.make_dims(**util.CFG["mid"])                            # V = 500
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgba_workspace_bytes(B(dims), 2, 3)
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

    def call(dm=dims, S=2, W=3, sup=1, wc=fake, al=fake, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 4 if outs is None else outs       # seq, seq_logp, score, trace
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgba_beam_search(None, B(dm), S, W, sup, wc, al, None if p is None else B(p), None if b is None else B(b),
                                  None if x is False else B(x), None if r is False else B(r), o[0], o[1], o[2], o[3], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(W=4, nbytes=need) == -4 and call(S=3, nbytes=need) == -4         # the workspace of (2, 3) serves neither
    assert call(S=1, W=1, nbytes=8) == -4 and call(W=8, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=-7, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=499, nbytes=8) == -4
    assert call(outs=[fake, fake, fake, None], nbytes=8) == -4                # trace may be NULL: the next check decides
    # XG_EINVAL: what the unconstrained search refuses ...
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
    assert call(S=0) == -1 and call(S=-2) == -1
    k10 = _mk(d, B=1 << 10)
    assert call(dm=k10, S=1 << 7, W=8, nbytes=8) == -4 and call(dm=k10, S=(1 << 7) + 1, W=8) == -1
    # ... and a null table or null masks: XG_EINVAL, and before the workspace is measured
    assert call(wc=None) == -1 and call(al=None) == -1 and call(wc=None, al=None) == -1
    assert call(wc=None, nbytes=8) == -1 and call(al=None, nbytes=8) == -1


# ---- the Python surface
def test_beam_captions_allowed_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    wc, al = torch.ones(d.V, dtype=torch.uint8), torch.full((d.B, S, d.L), ANY, dtype=torch.int64)
    with pytest.raises(NotImplementedError):                # train mode
        m.beam_captions_allowed(*f, pos, wc, al, beam_size=3)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.beam_captions_allowed(*f, pos, wc, al, beam_size=3)
    for bad in (pos.reshape(d.B * S, d.R), pos[:, :, 1:], pos.unsqueeze(0)):          # what beam_captions_per_video raises
        with pytest.raises(ValueError):
            m.beam_captions_allowed(*f, bad, wc, al, beam_size=3)
    for bad, a in ((pos[1:], al[1:]), (pos[:, :0], al[:, :0])):
        with pytest.raises(ValueError):
            m.beam_captions_allowed(*f, bad, wc, a, beam_size=3)
    for W in (0, 9, d.V + 1):
        with pytest.raises(ValueError):
            m.beam_captions_allowed(*f, pos, wc, al, beam_size=W)
    with pytest.raises(ValueError):
        m.beam_captions_allowed(*f, pos, wc, al, beam_size=3, suppress_token=d.V)
    # the table: (V,) uint8
    for bad in (wc[1:], wc.reshape(1, -1), wc.long(), wc.float(), wc.numpy(), None):
        with pytest.raises(ValueError, match="word_cat"):
            m.beam_captions_allowed(*f, pos, bad, al, beam_size=3)
    # the masks: (B,S,L) integers
    for bad in (al[:, :, 1:], al[:, 1:], al[1:], al.reshape(d.B * S, d.L), al.float(), al != 0, al.numpy()):
        with pytest.raises(ValueError, match="allow"):
            m.beam_captions_allowed(*f, pos, wc, bad, beam_size=3)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.beam_captions_allowed(*f, pos, wc, al, beam_size=3)


def test_word_category_table():
    from controllable_xgating_amd.data import word_categories, word_category_table
    wtoi = {"cat": 2, "runs": 3, "the": 4, "odd": 5, "<EOS>": 0, "UNK": 1}
    cat = word_categories({"NN": ["cat"], "VBZ": ["runs"], "DT": ["the"], "XX": ["odd"]}, wtoi)
    t = word_category_table(cat, wtoi, 8)
    assert t.dtype == np.uint8 and t.shape == (8,)
    assert t.tolist() == [0, 1, 3, 2, 9, 1, 1, 1]                  # index 0 -> 0, index 1 -> 1, unlisted indices unknown
    # indices 0 and 1 are fixed whatever the dicts say
    assert word_category_table({"a": 7, "b": 8}, {"a": 0, "b": 1}, 3).tolist() == [0, 1, 1]
    assert word_category_table({"a": 31}, {"a": 2}, 3).tolist() == [0, 1, 31]
    for bad in (32, 255, -1):
        with pytest.raises(ValueError):
            word_category_table({"a": bad}, {"a": 2}, 3)
    with pytest.raises(ValueError):
        word_category_table({"a": 3}, {"a": 3}, 3)                 # an index beyond the vocabulary


def test_allow_masks():
    from controllable_xgating_amd import allow_masks
    m = allow_masks([[[3, 2, -1], [9]], [[4, 0], []]], 4)
    assert m.dtype == torch.int64 and m.shape == (2, 2, 4)
    assert m.tolist() == [[[8, 4, ANY, 1], [512, 1, 1, 1]], [[16, 1, 1, 1], [1, 1, 1, 1]]]
    assert allow_masks([[3, 2], [5, 31]], 3).tolist() == [[[8, 4, 1]], [[32, 1 << 31, 1]]]          # [video][tag]
    t = torch.tensor([[[3, -1], [0, 31]]])
    assert allow_masks(t, 3).tolist() == [[[8, ANY, 1], [1, 1 << 31, 1]]]
    assert allow_masks(t.numpy().astype(np.int32), 2).tolist() == [[[8, ANY], [1, 1 << 31]]]
    assert allow_masks(t[0], 2).shape == (2, 1, 2)                                                  # (B,L')
    built = torch.tensor([[[0, ANY, 5]]])
    assert torch.equal(allow_masks(built, 3, built=True), built)                                    # passes through
    for bad, L in ((t, 1), ([[[1, 2, 3]]], 2), (torch.tensor([[[32]]]), 3), (torch.tensor([[[-2]]]), 3), ([[[32]]], 3), ([[[-2]]], 3),
                   (t.float(), 3), ([[[1], [2]], [[1]]], 3), ([], 3), (torch.zeros(2, 2, 2, 2, dtype=torch.int64), 3)):
        with pytest.raises(ValueError):
            allow_masks(bad, L)
    for bad in (built[:, :, :2], built[0], built.float()):
        with pytest.raises(ValueError):
            allow_masks(bad, 3, built=True)


def test_template_adherence():
    from controllable_xgating_amd import template_adherence
    wc = torch.tensor([0, 1, 2, 2, 3, 5], dtype=torch.uint8)       # category 4 has no word
    allow = torch.tensor([[[4, 8, 1], [ANY, 16, 0]]])              # group 0: 2, 3, end; group 1: any, the EMPTY category, zero
    seq = torch.tensor([[[[2, 4, 0], [3, 4, 5], [2, 0, 0], [2, 2, 0], [0, 5, 5]],
                         [[5, 5, 5], [1, 0, 0], [0, 0, 0], [4, 3, 2], [2, 2, 2]]]])
    got = template_adherence(seq, allow, wc)
    assert got.dtype == torch.bool and got.shape == (1, 2, 5)
    # group 0: the template itself; a word 5 where the end tag stands; the first 0 at a position of tag 3; tag 2 twice; a 0 at once
    # (what stands behind the first 0 is not read).  Group 1: both fallbacks admit every word
    assert got.tolist() == [[[True, False, False, False, False], [True, True, True, True, True]]]
    assert template_adherence(seq, torch.full((1, 2, 3), ANY), wc).all()
    with pytest.raises(ValueError):
        template_adherence(seq, allow[:, :1], wc)
    with pytest.raises(ValueError):
        template_adherence(seq[0], allow, wc)


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

    def beam_captions_allowed(self, fr, fo, fm, pos, word_cat, allow, beam_size=5, suppress_token=1, return_trace=False):
        self.calls.append((fr, fo, fm, pos, word_cat, allow, beam_size, suppress_token, return_trace))
        B, S = pos.shape[:2]
        n = B * S * beam_size * self.L
        return torch.arange(n).reshape(B, S, beam_size, self.L), torch.zeros(B, S, beam_size, self.L), torch.ones(B, S, beam_size)


def test_beam_captions_following_templates_hands_over_templates_as_masks():
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import allow_masks, beam_captions_following_templates
    for name in ("allow_masks", "beam_captions_following_templates", "template_adherence"):
        assert name in pkg.__all__
    B, S, L, R, K, W = 2, 2, 4, 6, 2, 3
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, S, L, R), _StubCap(L)
    tm = torch.tensor([[[3, 2, 0, 0], [9, 0, 0, 0]], [[4, 4, 4, 0], [2, 3, 0, 0]]])
    wc = torch.ones(11, dtype=torch.uint8)
    seq, lp, score, tscore = beam_captions_following_templates(pm, cap, fr, fo, fm, tm, wc, beam_size=W, suppress_token=-1)
    (a, b, c, t, collect, trim), = pm.calls
    assert a is fr and b is fo and c is fm and t is tm and collect is False and trim is False
    (a, b, c, pos, w_, al, w, sup, tr), = cap.calls
    assert a is fr and b is fo and c is fm and w_ is wc                       # un-repeated: the very tensors
    assert pos.shape == (B, S, R) and torch.equal(pos.reshape(B * S, R), pm.pos_feats)
    assert torch.equal(al, allow_masks(tm, L)) and (w, sup, tr) == (W, -1, False)       # constraints=None: the templates
    assert seq.shape == (B, S, W, L) and tscore.shape == (B, S) and torch.allclose(tscore, torch.full((B, S), -0.5 * L))
    cons = [[[-1, 3], [2]], [[5], [6, 7, 8]]]
    cap = _StubCap(L)
    beam_captions_following_templates(pm, cap, fr, fo, fm, tm, wc, constraints=cons)
    assert torch.equal(cap.calls[0][5], allow_masks(cons, L)) and cap.calls[0][6:8] == (5, 1)
    masks = torch.full((B, S, L), ANY)
    cap = _StubCap(L)
    beam_captions_following_templates(pm, cap, fr, fo, fm, tm, wc, constraints=masks, built=True)
    assert torch.equal(cap.calls[0][5], masks)


# ---- the oracle helper against itself
def test_constrain_by_hand():
    lp = np.log(np.array([[0.1, 0.2, 0.3, 0.4]]))
    wc = np.array([0, 1, 2, 2], np.uint8)
    ok = cao.allowed_words(wc, np.array([1 << 2, 1 << 1, 0, 1 << 7, ANY, 3]))
    assert ok.tolist() == [[False, False, True, True], [False, True, False, False], [True] * 4, [True] * 4, [True] * 4,
                           [True, True, False, False]]
    got = cao.constrain(lp, ok[0])
    np.testing.assert_allclose(got[0], [np.log(0.1 / 0.7) - 1000, np.log(0.2 / 0.7) - 1000, np.log(3 / 7), np.log(4 / 7)], atol=1e-12)
    assert cao.constrain(lp, ok[1])[0, 1] == 0.0                              # a single allowed word: exactly 0
    assert np.array_equal(cao.constrain(lp, ok[2]), lp)                       # every word allowed: untouched


def test_all_ones_masks_give_the_unconstrained_oracle_exactly():
    c = cao.case("tiny_s3w3")
    d, S, W = c["d"], c["S"], c["W"]
    for dtype in (torch.float32, torch.float64):
        want = cbo.beam_captions(c["P"], c["xr"], d.L, W, dtype=dtype)
        got = cao.allowed_beam_captions(c["P"], c["xr"], d.L, S, W, c["table"], np.full((d.B, S, d.L), ANY), dtype=dtype)
        for k in ("seq", "seq_logp", "score", "trace", "top_lp", "top_ix", "margin"):
            assert np.array_equal(got[k], want[k]), k


def _live(o, g):
    return [k for k in range(o["score"].shape[1]) if o["score"][g, k] > cao.LIVE]


def _adherent(seq, ok_g):
    """Every token of seq (L,) up to and including its first 0 is allowed: ok_g (L,V)."""
    for t, w in enumerate(seq):
        if not ok_g[t, w]:
            return False
        if w == 0:
            break
    return True


@pytest.mark.parametrize("name", ["tiny_s3w3", "tiny_s5w1", "odd_s2w2", "one_s6w2"])
def test_consequences_hold_in_float64(name):
    c, o = cao.case(name), cao.case_oracle(name)
    d, W = c["d"], c["W"]
    G = d.B * c["S"]
    ok = cao.allowed_words(c["table"], c["masks"])
    single = int(np.flatnonzero(c["table"] == cao.SINGLE)[0])
    seen = dict(live=0, forced=0, zero=0)
    for g in range(G):
        assert _live(o, g), g                                                  # every group has a live beam
        for k in _live(o, g):
            seq, lp = o["seq"][g, k], o["seq_logp"][g, k]
            seen["live"] += 1
            assert _adherent(seq, ok[g]), (g, k, seq)                          # 1. exact, no row excused
            if c["kinds"][g] == "plain" and c["n"][g] < d.L:                   # 2. exactly n words, the finish at step n
                n = c["n"][g]
                assert (seq[:n] != 0).all() and (seq[n:] == 0).all() and (lp[n + 1:] == 0).all(), (g, k, seq, n)
                assert [int(x) for x in c["table"][seq[:n]]] == c["tags"][g, :n].tolist()
                seen["forced"] += 1
            for t in range(d.L):                                               # 3. a single allowed word: lp exactly 0
                if c["masks"][g, t] == 1 << cao.SINGLE and (seq[:t] != 0).all():
                    assert seq[t] == single and lp[t] == 0.0, (g, k, t)
                    seen["zero"] += 1
    print(name, seen)
    assert seen["live"] >= G and (seen["forced"] or d.L == 1) and seen["zero"]
    # the oracle is admissible by its own rules
    assert cao.check_admissible(o["trace"], o["seq_logp"], o["score"], o["seq"], c["P"], c["xr"], d.L, W, c["table"], c["masks"]) >= G


# ---- preconditions of the GPU cases, on the float64 oracle alone
def test_case_table_names_every_edge():
    assert set(cao.PINNED) <= set(cao.CASES)
    for name, (cfg, S, W, seed, gain, tseed) in cao.CASES.items():
        c = cao.case(name)
        d, t, kinds = c["d"], c["table"], c["kinds"]
        G = d.B * S
        assert t.dtype == np.uint8 and t.shape == (d.V,) and t[0] == 0 and t[1] == 1 and (t[1:] != 0).all() and t.max() < 32, name
        assert (t == cao.SINGLE).sum() == 1 and (t == cao.EMPTY).sum() == 0 and (t == cao.PAIR).sum() == 2, name
        assert {"any", "two", "empty", "zero"} <= set(kinds), name                          # every special kind in every case
        ok = cao.allowed_words(t, c["masks"])
        for g in range(G):
            m, n = c["masks"][g], c["n"][g]
            assert 1 <= n <= d.L and (n < d.L or d.L == 1) and (m[n:] == 1).all(), (name, g)
            special = [x for x in m[:n] if bin(int(x)).count("1") != 1]
            want = {"any": [ANY], "zero": [0], "plain": [], "empty": []}.get(kinds[g])
            if kinds[g] == "two":
                assert len(special) == 1 and bin(int(special[0])).count("1") == 2, (name, g)
            else:
                assert special == want, (name, g, special)
            if kinds[g] == "empty":
                assert (m[:n] == 1 << cao.EMPTY).sum() == 1
            if kinds[g] in ("empty", "zero"):                                               # a fallback row: every word allowed
                at = int(np.flatnonzero((m == 0) | (m == 1 << cao.EMPTY))[0])
                assert ok[g, at].all()
            for x in m[:n]:                                                                 # no step leaves only the suppressed word
                assert cao.allowed_words(t, np.array([x]))[0, 2:].any()
    d = cao.case("tiny_s3w3")["d"]
    assert cao.CASES["tiny_s3w3"][2] == 3 > (cao.case("tiny_s3w3")["table"] == cao.PAIR).sum()     # a two-word row at W = 3
    assert cao.CASES["tiny_s5w1"][2] == 1 and cao.case("one_s6w2")["d"].L == 1 and cao.case("one_s6w2")["d"].V == 5
    assert cao.case("odd_s2w2")["d"].V == 37 and cao.case("mid_s4w5")["d"].B * 4 * 5 == 240
    assert 64 * 1024 < 4 * (cao.case("v20001")["d"].V + 8) <= 150 * 1024 and cao.case("v20001")["d"].V % 4 == 1
    assert 4 * (cao.case("v38500")["d"].V + 8) > 150 * 1024
    c1 = cao.case("c1_s2w5")["d"]
    assert (c1.B, c1.V, c1.R, c1.C) == (2, 20000, 512, 14) and d.V == 61


@pytest.mark.parametrize("name", ["tiny_s3w3", "tiny_s5w1", "mid_s4w5", "odd_s2w2", "one_s6w2", "short_row"])
def test_preconditions_of_the_gpu_cases(name):
    if name == "short_row":
        c = cao.short_row_case()
        masks, o = c["masks"], c["oracle"]
    else:
        c, masks, o = cao.case(name), cao.case(name)["masks"], cao.case_oracle(name)
    d, W = c["d"], c["W"]
    G = d.B * c["S"]
    ok = cao.allowed_words(c["table"], masks)                                               # (G,L,V)
    # a word that is not allowed lies below 400 before its -1000 in every row: the -1000 cannot climb past LIVE
    lp = o["logps"]                                                                         # (G,L,W,V), the -1000 applied
    raised = np.where(ok[:, :, None, :], -np.inf, lp + 1000)
    print("%s: largest disallowed lp before its -1000: %.3f" % (name, raised.max()))
    assert raised.max() < 400
    # the named edges are met by a LIVE slot of the float64 search
    tok = o["tokens"]
    if name == "short_row":
        pair = set(np.flatnonzero(c["table"] == cao.PAIR).tolist())
        assert all(set(tok[g, 0, :2].tolist()) == pair and tok[g, 0, 2] not in pair for g in range(G))
    elif name in ("tiny_s3w3", "mid_s4w5"):
        single = int(np.flatnonzero(c["table"] == cao.SINGLE)[0])
        assert any(masks[g, t] == 1 << cao.SINGLE and (o["seq"][g, k, :t + 1] != 0).all() and o["seq"][g, k, t] == single
                   for g in range(G) for t in range(d.L) for k in _live(o, g))              # a singleton step on a live beam
        assert any(masks[g, t] == 1 << cao.PAIR for g in range(G) for t in range(d.L))      # a two-word row
    else:
        assert any(k in c["kinds"] for k in ("empty", "zero"))                              # a fallback row
    if name in cao.PINNED or name == "short_row":
        pinned = int((o["margin"] >= cao.MARGIN).sum())
        print("%s: %d of %d groups pinned" % (name, pinned, G))
        assert 5 * pinned >= 4 * G
