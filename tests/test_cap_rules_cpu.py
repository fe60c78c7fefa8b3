"""CPU checks of the captioner's beam search under decoding rules: the C ABI of include/xgate_beam_rules.h (exports, version
through gcc, workspace sizes, every refusal without a GPU), the Python surface (every raise of SAModel.beam_captions_ruled,
control.length_scale_table, control.repeated_ngrams, data.bad_ending_ids, what control.beam_captions_ruled_with_templates hands
over), the oracle helper tests/cap_rules_oracle.py against itself and against tests/cap_allow_oracle.py with the rules off, and the
PRECONDITIONS of the cases tests/test_gpu_cap_rules.py runs, counted on the float64 oracle and pinned in the oracle file.  No compute
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
from tests import cap_allow_oracle as cao
from tests import cap_rules_oracle as cro
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
    txt = open(os.path.join(ROOT, "include", "xgate_beam_rules.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgbr_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgbr_beam_search", "xgbr_version", "xgbr_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgbr_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_beam_rules.h":
            assert not re.search(r"xgbr_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_and_struct_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_allow as nba
    from controllable_xgating_amd import _native_beam_rules as nbr
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xgate_beam_rules.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(XgDims), sizeof(XgBeamRules), '
                   'offsetof(XgBeamRules, min_length), offsetof(XgBeamRules, bad_end), offsetof(XgBeamRules, n_bad_end), '
                   'offsetof(XgBeamRules, length_scale), XGBR_VERSION, XGBR_MAX_BAD_END, XGBR_MAX_LENGTH, XGBA_VERSION, XG_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sr, o1, o2, o3, o4, ver, nbad, lmax, aver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                                        text=True).stdout.split())
    L = nbr.lib()
    assert ver == nbr.XGBR_VERSION == L.xgbr_version() == 1
    assert nbad == nbr.XGBR_MAX_BAD_END == 32 and lmax == nbr.XGBR_MAX_LENGTH
    assert aver == nba.XGBA_VERSION and xver == nv.XG_VERSION                   # the other versions did not move
    R = nbr.XgBeamRules
    assert sd == ctypes.sizeof(nv.XgDims) and sr == ctypes.sizeof(R)
    assert (o1, o2, o3, o4) == (R.min_length.offset, R.bad_end.offset, R.n_bad_end.offset, R.length_scale.offset)


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    """0 wherever the search without rules has size 0 (and beyond the longest caption), else that size plus two history blocks and
    the keys."""
    from controllable_xgating_amd import _native_beam_allow as nba
    from controllable_xgating_amd import _native_beam_rules as nbr
    Lr, La = nbr.lib(), nba.lib()
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
        r, a = Lr.xgbr_workspace_bytes(B(dm), S, W), La.xgba_workspace_bytes(B(dm), S, W)
        assert (r == 0) == (a == 0), (S, W, r, a)
        if r:
            M, L = dm.B * S * W, dm.T - 1
            assert a + 2 * 4 * M * L + 4 * M <= r <= a + 2 * 4 * M * L + 4 * M + 4 * 256, (S, W, r, a)
        zeros += r == 0
    assert 0 < zeros < len(dims)
    assert Lr.xgbr_workspace_bytes(None, 3, 3) == 0
    assert Lr.xgbr_workspace_bytes(B(_mk(d, L=nbr.XGBR_MAX_LENGTH)), 1, 1) > 0
    assert Lr.xgbr_workspace_bytes(B(_mk(d, L=nbr.XGBR_MAX_LENGTH + 1)), 1, 1) == 0


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_rules as nbr
    L = nbr.lib()
    d = pg.make_dims(**util.CFG["mid"])                            # V = 500, L = 7
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgbr_workspace_bytes(B(dims), 2, 3)
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

    def rules(n=0, mn=0, bad=None, nbad=0, scale=None):
        return nbr.XgBeamRules(n, mn, bad, nbad, scale)

    def call(dm=dims, S=2, W=3, sup=1, rl=Ellipsis, wc=fake, al=fake, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 5 if outs is None else outs       # seq, seq_logp, score, key, trace
        x = batch() if x is None else x
        r = run() if r is None else r
        rl = rules() if rl is Ellipsis else rl
        return L.xgbr_beam_search(None, B(dm), S, W, sup, None if rl is None else B(rl), wc, al, None if p is None else B(p),
                                  None if b is None else B(b), None if x is False else B(x), None if r is False else B(r),
                                  o[0], o[1], o[2], o[3], o[4], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(W=4, nbytes=need) == -4 and call(S=3, nbytes=need) == -4
    assert call(wc=None, al=None, nbytes=8) == -4                              # no template constraint: both NULL
    assert call(outs=[fake, fake, fake, None, None], nbytes=8) == -4           # key and trace may be NULL
    for ok in (rules(n=7), rules(mn=7), rules(n=1, mn=1), rules(bad=fake, nbad=32), rules(bad=fake, nbad=0), rules(scale=fake)):
        assert call(rl=ok, nbytes=8) == -4
    # XG_EINVAL: what the searches without rules refuse ...
    for W in (0, -1, 9, 64):
        assert call(W=W) == -1, W
    v5 = _mk(d, V=5)
    assert call(dm=v5, W=5, nbytes=8) == -4 and call(dm=v5, W=6) == -1        # W > V
    assert call(sup=500) == -1 and call(dm=v5, sup=5) == -1
    assert call(dm=_mk(d, B=0)) == -1 and call(dm=_mk(d, L=0)) == -1
    assert call(r=run(train=1)) == -1 and call(r=run(save=1)) == -1 and call(r=run(gemm_mode=1)) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(x=False) == -1 and call(r=False) == -1 and call(ws=None) == -1
    assert call(ws=fake + 16) == -1
    for i in range(4):
        st = [fake] * 4
        st[i] = None
        assert call(b=nv.XgBnState(*st)) == -1, i
    for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"):
        assert call(x=batch(**{k: None})) == -1, k
    for i in range(3):
        outs = [fake] * 5
        outs[i] = None
        assert call(outs=outs) == -1, i
    assert call(S=0) == -1 and call(S=-2) == -1
    k10 = _mk(d, B=1 << 10)
    assert call(dm=k10, S=1 << 7, W=8, nbytes=8) == -4 and call(dm=k10, S=(1 << 7) + 1, W=8) == -1
    # ... and the rules' own, each before the workspace is measured
    assert call(rl=None, nbytes=8) == -1
    assert call(rl=rules(n=-1), nbytes=8) == -1 and call(rl=rules(n=8), nbytes=8) == -1                # n > L = 7
    assert call(rl=rules(mn=-1), nbytes=8) == -1 and call(rl=rules(mn=8), nbytes=8) == -1
    assert call(rl=rules(bad=fake, nbad=-1), nbytes=8) == -1 and call(rl=rules(bad=fake, nbad=33), nbytes=8) == -1
    assert call(rl=rules(bad=None, nbad=1), nbytes=8) == -1
    assert call(wc=None, nbytes=8) == -1 and call(al=None, nbytes=8) == -1                             # exactly one NULL
    assert call(dm=_mk(d, L=nbr.XGBR_MAX_LENGTH + 1), nbytes=8) == -1 and call(dm=_mk(d, L=nbr.XGBR_MAX_LENGTH), nbytes=8) == -4


# ---- the Python surface
def test_beam_captions_ruled_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    wc, al = torch.ones(d.V, dtype=torch.uint8), torch.full((d.B, S, d.L), ANY, dtype=torch.int64)
    with pytest.raises(NotImplementedError):                # train mode
        m.beam_captions_ruled(*f, pos, beam_size=3)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.beam_captions_ruled(*f, pos, beam_size=3, no_repeat_ngram=2, min_length=2, bad_endings=[3, 4],
                              length_scale=torch.ones(d.L), word_cat=wc, allow=al)
    for bad in (pos.reshape(d.B * S, d.R), pos[:, :, 1:], pos.unsqueeze(0), pos[1:], pos[:, :0]):
        with pytest.raises(ValueError):
            m.beam_captions_ruled(*f, bad, beam_size=3)
    for W in (0, 9, d.V + 1):
        with pytest.raises(ValueError):
            m.beam_captions_ruled(*f, pos, beam_size=W)
    with pytest.raises(ValueError):
        m.beam_captions_ruled(*f, pos, beam_size=3, suppress_token=d.V)
    for n in (-1, d.L + 1):
        with pytest.raises(ValueError, match="no_repeat_ngram"):
            m.beam_captions_ruled(*f, pos, no_repeat_ngram=n)
        with pytest.raises(ValueError, match="min_length"):
            m.beam_captions_ruled(*f, pos, min_length=n)
    for bad in ([-1], [d.V], list(range(2, 35)), [[2, 3]], [2.0], torch.tensor([True])):
        with pytest.raises(ValueError, match="bad_endings"):
            m.beam_captions_ruled(*f, pos, bad_endings=bad)
    one = torch.ones(d.L)
    for bad in (one[1:], one.reshape(1, -1), one.long(), one * 0, one * 1.5, -one, one * float("nan"), one * float("inf"),
                torch.cat([one[:-1], torch.tensor([0.0])])):
        with pytest.raises(ValueError, match="length_scale"):
            m.beam_captions_ruled(*f, pos, length_scale=bad)
    with pytest.raises(ValueError, match="word_cat and allow"):
        m.beam_captions_ruled(*f, pos, word_cat=wc)
    with pytest.raises(ValueError, match="word_cat and allow"):
        m.beam_captions_ruled(*f, pos, allow=al)
    for bad in (wc[1:], wc.long(), wc.numpy()):
        with pytest.raises(ValueError, match="word_cat"):
            m.beam_captions_ruled(*f, pos, word_cat=bad, allow=al)
    for bad in (al[:, :, 1:], al[1:], al.float(), al != 0, al.numpy()):
        with pytest.raises(ValueError, match="allow"):
            m.beam_captions_ruled(*f, pos, word_cat=wc, allow=bad)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.beam_captions_ruled(*f, pos, beam_size=3)


def test_length_scale_table_by_hand():
    from controllable_xgating_amd import length_scale_table
    t = length_scale_table(4, 1.0)
    assert t.dtype == torch.float32 and t.shape == (4,)
    assert t.tolist() == [1.0, 0.5, float(np.float32(1 / 3)), 0.25]
    assert length_scale_table(3, 2.0).tolist() == [1.0, 0.25, float(np.float32(1 / 9))]
    w = length_scale_table(3, 0.7, "wu")
    assert w.tolist() == [float(np.float32((k / 6.0) ** -0.7)) for k in (6, 7, 8)] and w[0] == 1.0
    for kind in ("avg", "wu"):
        assert length_scale_table(5, 0.0, kind).tolist() == [1.0] * 5
        big = length_scale_table(512, 3.0, kind)
        assert bool(((big > 0) & (big <= 1)).all()) and bool((big[:-1] >= big[1:]).all())
    for bad in (dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=1.0, kind="x")):
        with pytest.raises(ValueError):
            length_scale_table(4, **bad)
    with pytest.raises(ValueError):
        length_scale_table(0, 1.0)


def test_repeated_ngrams_against_a_python_loop():
    from controllable_xgating_amd import repeated_ngrams
    rng = np.random.RandomState(3)
    seq = rng.randint(0, 4, (3, 2, 5, 7))
    seq[0, 0, 0] = [2, 2, 0, 2, 2, 2, 2]                            # what stands behind the first 0 is not read
    seq[0, 0, 1] = [1, 2, 3, 1, 2, 3, 1]                            # no 0 at all
    seq[0, 0, 2] = 0
    for n in (1, 2, 3, 6, 7, 9):
        got = repeated_ngrams(torch.from_numpy(seq), n)
        assert got.dtype == torch.bool and got.shape == seq.shape[:-1]
        want = np.array([cro.has_repeat(s, n) for s in seq.reshape(-1, 7)]).reshape(seq.shape[:-1])
        assert np.array_equal(got.numpy(), want), n
        assert want.any() or n >= 4
    assert repeated_ngrams(torch.tensor([2, 2, 0, 2, 2, 2, 2]), 1).item() is True
    assert repeated_ngrams(torch.tensor([2, 2, 0, 2, 2, 2, 2]), 2).item() is False
    assert repeated_ngrams(torch.tensor([5, 5, 5, 0]), 2).item() is True                # "a a a" holds "a a" twice
    with pytest.raises(ValueError):
        repeated_ngrams(torch.from_numpy(seq), 0)


def test_bad_ending_ids():
    from controllable_xgating_amd.data import BAD_ENDINGS, bad_ending_ids
    assert BAD_ENDINGS == ("a", "an", "the", "in", "for", "at", "of", "with", "before", "after", "on", "upon", "near", "to", "is",
                           "are", "am")
    wtoi = {"the": 4, "cat": 2, "a": 9, "with": 3, "<EOS>": 0}
    assert bad_ending_ids(wtoi) == [9, 4, 3]                        # the list's order; missing words skipped
    assert bad_ending_ids(wtoi, ["cat", "dog", "cat"]) == [2] and bad_ending_ids({}, ["a"]) == []
    assert len(BAD_ENDINGS) <= 32


class _StubPos:
    def __init__(self, B, S, L, R):
        self.pos_feats = torch.arange(B * S * R, dtype=torch.float32).reshape(B * S, R)
        self.B, self.S, self.L, self.calls = B, S, L, []

    def sample_forced(self, fr, fo, fm, templates, collect_states=False, trim=False):
        self.calls.append((fr, fo, fm, templates, collect_states, trim))
        return torch.full((self.B, self.S, self.L), -0.5), None, None, self.pos_feats


class _StubCap:
    def __init__(self, L):
        self.L, self.calls = L, []

    def beam_captions_ruled(self, fr, fo, fm, pos, **kw):
        self.calls.append((fr, fo, fm, pos, kw))
        B, S = pos.shape[:2]
        W = kw.get("beam_size", 5)
        return (torch.zeros(B, S, W, self.L, dtype=torch.int64), torch.zeros(B, S, W, self.L), torch.ones(B, S, W),
                torch.full((B, S, W), 2.0))


def test_beam_captions_ruled_with_templates_hands_over():
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import allow_masks, beam_captions_ruled_with_templates
    for name in ("length_scale_table", "repeated_ngrams", "beam_captions_ruled_with_templates"):
        assert name in pkg.__all__
    B, S, L, R, K, W = 2, 2, 4, 6, 2, 3
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, S, L, R), _StubCap(L)
    tm = torch.tensor([[[3, 2, 0, 0], [9, 0, 0, 0]], [[4, 4, 4, 0], [2, 3, 0, 0]]])
    scale = torch.ones(L)
    out = beam_captions_ruled_with_templates(pm, cap, fr, fo, fm, tm, beam_size=W, no_repeat_ngram=2, min_length=1, bad_endings=[3],
                                             length_scale=scale)
    assert len(out) == 5 and out[0].shape == (B, S, W, L) and torch.equal(out[3], torch.full((B, S, W), 2.0))
    assert torch.allclose(out[4], torch.full((B, S), -0.5 * L))
    (a, b, c, t, collect, trim), = pm.calls
    assert a is fr and b is fo and c is fm and t is tm and collect is False and trim is False
    (a, b, c, pos, kw), = cap.calls
    assert a is fr and b is fo and c is fm and pos.shape == (B, S, R) and torch.equal(pos.reshape(B * S, R), pm.pos_feats)
    assert kw["word_cat"] is None and kw["allow"] is None and kw["length_scale"] is scale
    assert {k: kw[k] for k in ("beam_size", "no_repeat_ngram", "min_length", "bad_endings")} == dict(
        beam_size=W, no_repeat_ngram=2, min_length=1, bad_endings=[3])
    wc = torch.ones(11, dtype=torch.uint8)
    cap = _StubCap(L)
    beam_captions_ruled_with_templates(pm, cap, fr, fo, fm, tm, wc, no_repeat_ngram=1)
    assert cap.calls[0][4]["word_cat"] is wc and torch.equal(cap.calls[0][4]["allow"], allow_masks(tm, L))
    cons = [[[-1, 3], [2]], [[5], [6, 7, 8]]]
    cap = _StubCap(L)
    beam_captions_ruled_with_templates(pm, cap, fr, fo, fm, tm, wc, constraints=cons)
    assert torch.equal(cap.calls[0][4]["allow"], allow_masks(cons, L))
    with pytest.raises(ValueError):
        beam_captions_ruled_with_templates(pm, _StubCap(L), fr, fo, fm, tm, constraints=cons)


# ---- the oracle helper against itself
def test_ban_sets_by_hand():
    b = cro.ban_sets
    assert b([], 1) == set() and b([5], 2) == set() and b([5, 6], 3) == set()              # t < n
    assert b([5, 6, 5], 1) == {5, 6} and b([0, 0], 1) == {0}                               # n = 1: every word of the history
    assert b([7, 7], 2) == {7} and b([7, 7, 7], 2) == {7}                                  # "a a a" at n = 2: a, once
    assert b([1, 2, 3, 1, 2], 3) == {3} and b([1, 2, 3, 1, 2], 2) == {3} and b([1, 2, 3, 1], 2) == {2}
    assert b([1, 2, 1, 3, 1], 2) == {2, 3}
    assert b([1, 2, 3, 4], 2) == set() and b([1, 2, 3], 3) == set()
    assert b([], 0, min_length=1) == {0} and b([4], 0, min_length=1) == set() and b([4, 4], 0, min_length=3) == {0}
    assert b([4], 0, bad_end=(4,)) == {0} and b([4, 5], 0, bad_end=(4,)) == set() and b([], 0, bad_end=(0,)) == set()
    assert b([4, 0], 1, min_length=3, bad_end=(0,)) == {4, 0}                              # word 0 named by three rules: once
    assert len(b([0, 4], 1, min_length=3, bad_end=(4,))) == 2
    m = cro.ban_mask(np.array([[[7, 7], [1, 2]]]), 9, cro.rules(n=2, min_length=3))
    assert m.shape == (1, 2, 9) and np.flatnonzero(m[0, 0]).tolist() == [0, 7] and np.flatnonzero(m[0, 1]).tolist() == [0]


def test_histories_of_a_trace():
    tr = np.zeros((1, 3, 2, 2), np.int32)
    tr[0, 0, :, 0], tr[0, 1, :, 0], tr[0, 2, :, 0] = [5, 6], [7, 8], [9, 4]
    tr[0, 1, :, 1], tr[0, 2, :, 1] = [1, 1], [1, 0]
    h = cro.histories_of(tr)
    assert h[0, 0].tolist() == [[0, 0, 0], [0, 0, 0]] and h[0, 1].tolist() == [[5, 0, 0], [6, 0, 0]]
    assert h[0, 2].tolist() == [[6, 7, 0], [6, 8, 0]]


@pytest.mark.parametrize("masks", [True, False])
def test_rules_off_give_the_oracles_without_rules_exactly(masks):
    c = cao.case("tiny_s3w3")
    d, S, W = c["d"], c["S"], c["W"]
    for dtype in (torch.float32, torch.float64):
        if masks:
            want = cao.allowed_beam_captions(c["P"], c["xr"], d.L, S, W, c["table"], c["masks"], dtype=dtype)
            got = cro.ruled_beam_captions(c["P"], c["xr"], d.L, S, W, cro.OFF, c["table"], c["masks"], dtype=dtype)
        else:
            want = cao.allowed_beam_captions(c["P"], c["xr"], d.L, S, W, c["table"], np.full((d.B, S, d.L), ANY), dtype=dtype)
            got = cro.ruled_beam_captions(c["P"], c["xr"], d.L, S, W, dtype=dtype)
        for k in ("seq", "seq_logp", "score", "trace", "top_lp", "top_ix", "margin", "logps"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["key"], got["score"])
        # an n-gram as long as the caption can never repeat: the rule is on and bans nothing
        same = cro.ruled_beam_captions(c["P"], c["xr"], d.L, S, W, cro.rules(n=d.L), *((c["table"], c["masks"]) if masks else ()),
                                       dtype=dtype)
        assert np.array_equal(same["trace"], got["trace"]) and np.array_equal(same["score"], got["score"])


# ---- preconditions of the GPU cases, counted in float64 and pinned in the oracle file
def test_case_table_names_every_edge():
    assert set(cro.PINS) == set(cro.REPETITION) | set(cro.LENGTH) and set(cro.TRACE_CASES) <= set(cro.CASES)
    d = {n: cro.case(n)["d"] for n in cro.CASES}
    assert d["tiny_n1"].L == 12 and d["odd_n1"].L == 9 and d["odd_n1"].V == 37 and d["mid_n3"].L == 12
    assert d["one_n1"].L == 1 and d["one_n1"].V == 5
    assert 64 * 1024 < 4 * (d["v20001_n2"].V + 8) <= 150 * 1024 and d["v20001_n2"].V % 4 == 1 and d["v20001_n2"].L == 8
    assert 4 * (d["v38500_n2"].V + 8) > 150 * 1024 and d["v38500_n2"].L == 8
    c1 = d["c1_n3"]
    assert (c1.B, c1.V, c1.R, c1.L) == (2, 20000, 512, 20) and cro.CASES["c1_n3"][1:3] == (2, 5)
    assert [cro.CASES[n][5] for n in cro.TRACE_CASES] == [1, 2, 1, 3, 1, 2, 2, 3]


@pytest.mark.parametrize("name", list(cro.PINS))
def test_preconditions_of_the_gpu_cases(name):
    got, pin = cro.count_pins(name), cro.PINS[name]
    print(name, got)
    assert got == pin
    G = pin["groups"]
    assert pin["live_best"] == G                                              # every group of the ruled search keeps a live best beam
    if name in cro.REPETITION:
        assert pin["plain_rep"] == G and pin["ruled_rep"] == 0                # every plain group repeats; no ruled live beam does
    if name in cro.LENGTH:
        assert pin["plain_short"] == G and pin["ruled_short"] == 0
    c, o = cro.case(name), cro.oracle64(name)
    # the oracle is admissible by its own rules
    assert cro.check_admissible(o["trace"], o["seq_logp"], o["score"], o["key"], o["seq"], c["P"], c["xr"], c["d"].L, c["W"], c["rl"]) >= G


def test_preconditions_of_the_bad_endings_and_length_scale_cases():
    c = cro.case(cro.BAD_END_CASE)
    d, S, W = c["d"], c["S"], c["W"]
    plain = cro.oracle64(cro.BAD_END_CASE, False)
    assert tuple(cro.live_endings(plain)) == cro.PINNED_BAD_END and len(cro.PINNED_BAD_END) >= 1
    assert 0 not in cro.PINNED_BAD_END and 1 not in cro.PINNED_BAD_END
    o = cro.ruled_beam_captions(c["P"], c["xr"], d.L, S, W, cro.rules(bad_end=cro.PINNED_BAD_END), dtype=torch.float64)
    assert not set(cro.live_endings(o)) & set(cro.PINNED_BAD_END) and (o["score"][:, 0] > cro.LIVE).all()
    assert any(len(cro.words_of(s)) == 0 for s in o["seq"][:, 0])             # the empty caption is untouched by this rule
    for form, pin in cro.PINNED_REORDERED.items():
        s = cro.scale_oracle64(form)
        assert cro.reordered_groups(s) == pin and (s["score"][:, 0] > cro.LIVE).all()
        rl = cro.rules(scale=cro.scale_table(d.L, form))
        assert cro.check_admissible(s["trace"], s["seq_logp"], s["score"], s["key"], s["seq"], c["P"], c["xr"], d.L, W, rl) >= d.B * S
    assert cro.PINNED_REORDERED["avg1"] >= 1
