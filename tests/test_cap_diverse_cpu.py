"""CPU checks of the captioner's diverse beam search (include/xgate_beam_diverse.h): the oracle (tests/cap_diverse_oracle.py) against
itself -- one group is the plain search, no penalty repeats it in every group, a penalty of 1000 keeps the live words of a pair's
groups apart, the kernel's top-N route selects what the full rows select --, the preconditions of every GPU case pinned as counts
on the float64 oracle, the C ABI (exports, version, workspace sizes, every refusal in order without a GPU), the raises of
SAModel.beam_captions_diverse and control.diverse_beam_captions_with_templates over stub models.  No compute on a GPU."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_beam_oracle as cbo
from tests import cap_diverse_oracle as cdo
from tests import util
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


@functools.lru_cache(maxsize=None)
def _oracle(name, lam, dtype=torch.float64, groups=None, top_n_only=False):
    d, P, x, pos, Gd, Wg = cdo.case(name)
    if groups is not None:
        Gd, Wg = groups
    torch.set_num_threads(8)
    return d, Gd, Wg, cdo.beam_captions_diverse(P, cdo.repeated(x, pos), d.L, Gd, Wg, lam, dtype=dtype, top_n_only=top_n_only)


@functools.lru_cache(maxsize=None)
def _plain(name, W, dtype):
    d, P, x, pos, _, _ = cdo.case(name)
    return cbo.beam_captions(P, cdo.repeated(x, pos), d.L, W, dtype=dtype)


# ---- the oracle against itself
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["tiny_s3g2w2", "eos_s2g3w1", "odd_s2g2w2"])
def test_one_group_is_the_plain_search(name, dtype):
    W = 3
    p = _plain(name, W, dtype)
    for lam in (0.0, 0.7, 1000.0):
        d, _, _, o = _oracle(name, lam, dtype, (1, W))
        assert np.array_equal(o["trace"], p["trace"]) and np.array_equal(o["seq"][:, 0], p["seq"])
        assert np.array_equal(o["logp"][:, 0], p["seq_logp"]) and np.array_equal(o["score"][:, 0], p["score"]) and o["changed"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["tiny_s3g2w2", "eos_s2g2w2", "mid_s2g4w2"])
def test_without_a_penalty_every_group_is_the_plain_search(name, dtype):
    """Every group selects what the plain search selects and its values agree to rounding (the eager oracle's products give a row
    other last bits at another place among other rows); the rule itself is exact on given rows:
    tests/test_pos_diverse_cpu.test_the_rule_is_exact_on_given_rows."""
    d, Gd, Wg, o = _oracle(name, 0.0, dtype)
    p = _plain(name, Wg, dtype)
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    assert o["changed"] == 0
    for j in range(Gd):
        assert np.array_equal(o["seq"][:, j], p["seq"])
        np.testing.assert_allclose(o["logp"][:, j], p["seq_logp"], atol=tol)
        np.testing.assert_allclose(o["score"][:, j], p["score"], atol=d.L * tol)
        tr = o["trace"][:, :, j * Wg:(j + 1) * Wg].copy()
        tr[..., 1] -= j * Wg
        assert np.array_equal(tr, p["trace"])


@pytest.mark.parametrize("name", [n for n in cdo.CASES if n != "v20001_g2w3"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 1000.0])
def test_top_n_rows_give_the_selection_of_the_full_rows(name, lam):
    """The lemma on the model's own rows, in the kernel's arithmetic (float32): cutting every row to its N best words before the
    merge changes nothing, bit for bit."""
    d, Gd, Wg, full = _oracle(name, lam, torch.float32)
    _, _, _, top = _oracle(name, lam, torch.float32, None, True)
    for k in ("seq", "logp", "score", "trace"):
        assert np.array_equal(full[k], top[k]), k
    if lam == 1000.0:
        assert full["disjoint"] and top["disjoint"]


# ---- the preconditions of the GPU cases (tests/test_gpu_cap_diverse.py), as counts on the float64 oracle at lambda = 0.5 / 1000:
# (group steps whose selection the penalty changes, dead slots whose word a later live slot takes, pairs whose groups finish at
# different steps, pairs with a float64 margin >= 1e-3)
PRE = {
    "tiny_s3g2w2": ((90, 0, 0, 10), (90, 0, 0, 10)),
    "tiny_s1g3w1": ((59, 0, 0, 4), (59, 0, 0, 4)),
    "eos_s2g3w1": ((26, 17, 10, 10), (34, 21, 10, 10)),
    "eos_s2g2w2": ((56, 0, 8, 7), (55, 0, 10, 7)),
    "mid_s2g2w4": ((112, 0, 0, 17), (168, 0, 0, 14)),
    "mid_s2g4w2": ((502, 0, 0, 2), (502, 0, 0, 2)),
    "mideos_s2g4w2": ((382, 15, 24, 10), (467, 6, 24, 11)),
    "odd_s2g2w2": ((24, 0, 0, 5), (24, 0, 0, 5)),
    "one_s2g2w2": ((2, 0, 0, 2), (2, 0, 0, 2)),
    "tiny_s2g8w1": ((364, 0, 0, 8), (419, 0, 0, 5)),
    "v20001_g2w3": ((14, 0, 0, 1), (14, 0, 0, 1)),
}


def counts(o):
    apart = sum(1 for r in o["finish"] if len({tuple(g) for g in r}) > 1)
    return o["changed"], o["dead_reused"], apart, int((o["margin"] >= cbo.MARGIN).sum())


@pytest.mark.parametrize("name", list(cdo.CASES))
def test_gpu_case_preconditions(name):
    assert set(PRE) == set(cdo.CASES)
    dd, _, _, _, S, Gd, Wg = cdo.CASES[name]
    assert S >= 1 and 1 <= Gd * Wg <= min(8, dd["V"])
    for lam, want in zip((cdo.LAMBDA, 1000.0), PRE[name]):
        d, _, _, o = _oracle(name, lam)
        assert counts(o) == want, (name, lam, counts(o))
        assert want[0] >= 1 and want[3] >= 1                      # the penalty changes a selection; a margin pins a pair
        assert o["near_dead"] > 400                               # no live sum comes near -500
        if lam == 1000.0:
            assert o["disjoint"]
    # over the cases: groups that finish at different steps, and a dead slot's word taken by a later group's live slot
    assert PRE["eos_s2g3w1"][0][1] >= 1 and PRE["mideos_s2g4w2"][0][1] >= 1 and PRE["eos_s2g2w2"][0][2] >= 1
    c = cdo.CASES
    assert (c["tiny_s3g2w2"][4:], c["tiny_s1g3w1"][4:], c["mid_s2g2w4"][4:], c["mid_s2g4w2"][4:]) == ((3, 2, 2), (1, 3, 1), (2, 2, 4), (2, 4, 2))
    assert c["odd_s2g2w2"][5:] == (2, 2) and c["one_s2g2w2"][5:] == (2, 2) and c["one_s2g2w2"][0]["V"] == 5
    assert c["tiny_s2g8w1"][5:] == (8, 1) and c["v20001_g2w3"][5:] == (2, 3)
    v = c["v20001_g2w3"][0]
    assert (v["V"], v["R"], v["A"], v["E"]) == (20001, 512, 1536, 468) and 64 * 1024 < 4 * (v["V"] + 8) <= 150 * 1024


def test_admissibility_check_accepts_the_oracle_and_refuses_a_wrong_search():
    d, P, x, pos, Gd, Wg = cdo.case("eos_s2g3w1")
    xr = cdo.repeated(x, pos)
    _, _, _, o = _oracle("eos_s2g3w1", cdo.LAMBDA, torch.float32)
    n, live = cdo.check_admissible(o["trace"], o["logp"], o["score"], o["seq"], P, xr, d.L, Gd, Wg, cdo.LAMBDA)
    assert n >= d.B * 2 * Gd and live.shape == (d.B * 2, d.L, Gd * Wg)
    with pytest.raises(AssertionError):                           # the same search judged under another penalty
        cdo.check_admissible(o["trace"], o["logp"], o["score"], o["seq"], P, xr, d.L, Gd, Wg, 3.0)
    with pytest.raises(AssertionError):                           # a parent outside the slot's group
        bad = o["trace"].copy()
        bad[:, 1, 1, 1] = 0
        cdo.check_admissible(bad, o["logp"], o["score"], o["seq"], P, xr, d.L, Gd, Wg, cdo.LAMBDA)


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_beam_diverse.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgdb_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgdb_beam_search", "xgdb_version", "xgdb_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgdb_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_beam_diverse.h":
            assert not re.search(r"xgdb_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam as nb
    from controllable_xgating_amd import _native_beam_diverse as ndb
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_beam_diverse.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGDB_VERSION, XG_VERSION, XGDB_MAX_BEAM);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, xver, nmax = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = ndb.lib()
    assert ver == ndb.XGDB_VERSION == L.xgdb_version() == 1 and xver == nv.XG_VERSION
    assert nmax == ndb.XGDB_MAX_BEAM == nb.XGCB_MAX_BEAM == 8
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native_beam_control as nbc
    from controllable_xgating_amd import _native_beam_diverse as ndb
    L, Lc = ndb.lib(), nbc.lib()
    B = ctypes.byref
    d = pg.make_dims(**util.CFG["mid"])
    size = lambda S, Gd, Wg, dm=None: L.xgdb_workspace_bytes(B(_mk(d) if dm is None else dm), S, Gd, Wg)      # noqa: E731
    for S in (1, 3):
        for W in range(1, 9):                                     # one group: the rows-per-video search's workspace
            assert size(S, 1, W) == Lc.xgbc_workspace_bytes(B(_mk(d)), S, W) > 0
    # the same N in more groups: only done_n grows, by one int32 per pair and extra group (regions are rounded up)
    for Gd, Wg in ((2, 4), (4, 2), (8, 1)):
        assert 0 <= size(3, Gd, Wg) - size(3, 1, 8) <= 4 * d.B * 3 * (Gd - 1) + 512
    assert all(size(S, 2, 2) < size(S + 1, 2, 2) for S in range(1, 6)) and size(2, 2, 2) < size(2, 2, 3) < size(2, 2, 4)
    for S, Gd, Wg in ((0, 2, 2), (-1, 2, 2), (2, 0, 2), (2, 2, 0), (2, -1, 2), (2, 2, -1), (2, 3, 3), (2, 9, 1), (2, 1, 9),
                      (2, 1 << 16, 1 << 16), (2, 1 << 30, 2)):
        assert size(S, Gd, Wg) == 0, (S, Gd, Wg)
    assert L.xgdb_workspace_bytes(None, 2, 2, 2) == 0
    for bad in (_mk(d, B=0), _mk(d, L=0), _mk(d, R=0), _mk(d, V=1)):
        assert size(2, 2, 2, bad) == 0
    v5 = _mk(d, V=5)
    assert size(2, 5, 1, v5) > 0 and size(2, 2, 2, v5) > 0 and size(2, 2, 3, v5) == 0 and size(2, 3, 2, v5) == 0       # N > V
    k10 = _mk(d, B=1 << 10)
    assert size(1 << 7, 4, 2, k10) > 0 and size((1 << 7) + 1, 4, 2, k10) == 0                                          # 2^20 rows


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam_diverse as ndb
    L = ndb.lib()
    d = pg.make_dims(**util.CFG["mid"])                            # V = 500
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgdb_workspace_bytes(B(dims), 2, 2, 2)
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

    def call(dm=dims, S=2, Gd=2, Wg=2, lam=0.5, sup=1, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 4 if outs is None else outs       # seq, seq_logp, score, trace
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgdb_beam_search(None, B(dm), S, Gd, Wg, lam, sup, None if p is None else B(p), None if b is None else B(b),
                                  None if x is False else B(x), None if r is False else B(r), o[0], o[1], o[2], o[3], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(Wg=3, nbytes=need) == -4 and call(S=3, nbytes=need) == -4       # the workspace of (2, 2, 2) serves neither
    assert call(S=1, Gd=1, Wg=1, nbytes=8) == -4 and call(Gd=8, Wg=1, nbytes=8) == -4 and call(Gd=1, Wg=8, nbytes=8) == -4
    assert call(lam=0.0, nbytes=8) == -4 and call(lam=-0.0, nbytes=8) == -4 and call(lam=1000.0, nbytes=8) == -4 and call(lam=3e38, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=499, nbytes=8) == -4
    assert call(outs=[fake, fake, fake, None], nbytes=8) == -4                # trace may be NULL: the next check decides
    # XG_EINVAL, all of it ahead of the workspace's size (nbytes = 8 would otherwise give -4): what the rows-per-video search
    # refuses ...
    v5 = _mk(d, V=5)
    assert call(dm=v5, Gd=5, Wg=1, nbytes=8) == -4 and call(dm=v5, Gd=2, Wg=3, nbytes=8) == -1        # N > V
    assert call(sup=500, nbytes=8) == -1 and call(dm=v5, sup=5, nbytes=8) == -1
    assert call(dm=_mk(d, B=0), nbytes=8) == -1 and call(dm=_mk(d, L=0), nbytes=8) == -1
    assert call(r=run(train=1), nbytes=8) == -1 and call(r=run(save=1), nbytes=8) == -1 and call(r=run(gemm_mode=1), nbytes=8) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(x=False) == -1 and call(r=False) == -1 and call(ws=None) == -1
    assert call(ws=fake + 16, nbytes=8) == -1                                 # the workspace is 256-byte aligned
    for i in range(3):
        outs = [fake] * 4
        outs[i] = None
        assert call(outs=outs, nbytes=8) == -1, i
    assert call(S=0, nbytes=8) == -1 and call(S=-2, nbytes=8) == -1
    k10 = _mk(d, B=1 << 10)
    assert call(dm=k10, S=1 << 7, Gd=4, Wg=2, nbytes=8) == -4 and call(dm=k10, S=(1 << 7) + 1, Gd=4, Wg=2, nbytes=8) == -1
    # ... then the new arguments
    for Gd, Wg in ((0, 2), (2, 0), (-1, 2), (2, -3), (3, 3), (9, 1), (1, 9), (1 << 16, 1 << 16)):
        assert call(Gd=Gd, Wg=Wg, nbytes=8) == -1, (Gd, Wg)
    for lam in (-0.5, -1e-30, float("inf"), float("-inf"), float("nan")):
        assert call(lam=lam, nbytes=8) == -1, lam


# ---- the Python surface
def test_beam_captions_diverse_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])                           # V = 61
    S = 3
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos = torch.zeros(d.B, S, d.R)
    with pytest.raises(NotImplementedError):                # train mode
        m.beam_captions_diverse(*f, pos, 2, 2)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.beam_captions_diverse(*f, pos, 2, 2)
    for bad in (pos.reshape(d.B * S, d.R), pos[1:], pos[:, :, 1:], pos[:, :0], pos.unsqueeze(0)):
        with pytest.raises(ValueError, match="pos_feats"):
            m.beam_captions_diverse(*f, bad, 2, 2)
    for Gd, Wg in ((0, 2), (2, 0), (-1, -1), (3, 3), (9, 1), (1, 9), (2, 5)):
        with pytest.raises(ValueError, match="groups"):
            m.beam_captions_diverse(*f, pos, Gd, Wg)
    for lam in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="diversity"):
            m.beam_captions_diverse(*f, pos, 2, 2, diversity=lam)
    with pytest.raises(ValueError, match="suppress_token"):
        m.beam_captions_diverse(*f, pos, 2, 2, suppress_token=d.V)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.beam_captions_diverse(*f, pos, 2, 2)


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

    def beam_captions_diverse(self, fr, fo, fm, pos, groups, group_size, diversity=0.5, suppress_token=1, return_trace=False):
        self.calls.append((fr, fo, fm, pos, groups, group_size, diversity, suppress_token, return_trace))
        B, S = pos.shape[:2]
        shape = (B, S, groups, group_size, self.L)
        return torch.zeros(shape, dtype=torch.int64), torch.zeros(shape), torch.ones(shape[:4])

    def sample(self, *a, **k):
        raise AssertionError("another path ran")

    beam_captions = beam_captions_per_video = sample_per_video = sample


def test_diverse_beam_captions_with_templates_hands_the_videos_over_once():
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import diverse_beam_captions_with_templates
    assert "diverse_beam_captions_with_templates" in pkg.__all__
    B, S, L, R, K, Gd, Wg = 3, 4, 5, 6, 2, 2, 3
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, S, L, R), _StubCap(L)
    tm = torch.zeros(B, S, L, dtype=torch.int64)
    seq, lp, score, tscore = diverse_beam_captions_with_templates(pm, cap, fr, fo, fm, tm, Gd, Wg, diversity=0.25, suppress_token=-1)
    (a, b, c, t, collect, trim), = pm.calls
    assert a is fr and b is fo and c is fm and t is tm and collect is False and trim is False
    (a, b, c, pos, g, w, lam, sup, tr), = cap.calls
    assert a is fr and b is fo and c is fm                                    # un-repeated: the very tensors
    assert pos.shape == (B, S, R) and torch.equal(pos.reshape(B * S, R), pm.pos_feats)
    assert (g, w, lam, sup, tr) == (Gd, Wg, 0.25, -1, False)
    assert seq.shape == (B, S, Gd, Wg, L) and lp.shape == seq.shape and score.shape == (B, S, Gd, Wg)
    assert tscore.shape == (B, S) and torch.allclose(tscore, torch.full((B, S), -0.5 * L))
    cap = _StubCap(L)
    diverse_beam_captions_with_templates(pm, cap, fr, fo, fm, tm, Gd, Wg)
    assert cap.calls[0][6:8] == (0.5, 1)                                      # the defaults of beam_captions_diverse
