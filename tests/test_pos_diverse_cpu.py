"""CPU checks of diverse POS beam search (include/xgate_pos_beam_diverse.h): the group oracle (tests/pos_diverse_oracle.py) against
itself -- Gd = 1 is the plain search, lambda = 0 repeats it in every group, lambda = 1000 keeps the live tags of a video's groups
apart, in float32 and float64 --, the top-N lemma on tie-heavy rows, the preconditions of every GPU case pinned as counts on the
float64 oracle, the C ABI (exports, version, workspace sizes, every refusal without a GPU), the raises of
PosModel.beam_templates_diverse and control.caption_beam_diverse over stub models.  No compute on a GPU."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pos_beam_oracle as pbo
from tests import pos_control_oracle as pco
from tests import pos_diverse_oracle as pdo
from tests import pos_oracle as po
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _inputs(x, dtype):
    return [torch.from_numpy(x[k]).to(dtype) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


@functools.lru_cache(maxsize=None)
def _oracle(name, lam, dtype=torch.float64, groups=None):
    d, P, run, x, Gd, Wg = pdo.case(name)
    if groups is not None:
        Gd, Wg = groups
    torch.set_num_threads(8)
    return d, Gd, Wg, pdo.beam_templates_diverse(po.to_torch(P, dtype), po.to_torch(run, dtype), *_inputs(x, dtype), d.L, Gd, Wg, lam)


@functools.lru_cache(maxsize=None)
def _plain(name, W, dtype):
    d, P, run, x, _, _ = pdo.case(name)
    return pbo.beam_templates(po.to_torch(P, dtype), po.to_torch(run, dtype), *_inputs(x, dtype), d.L, W)


# ---- the oracle against itself: the three consequences of the rule
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["tiny_g2w2", "eos_g3w1", "c65"])
def test_one_group_is_the_plain_search(name, dtype):
    W = 3
    p = _plain(name, W, dtype)
    for lam in (0.0, 0.7, 1000.0):
        d, _, _, o = _oracle(name, lam, dtype, (1, W))
        assert np.array_equal(o["trace"], p["trace"]) and np.array_equal(o["templates"][:, 0], p["templates"])
        assert np.array_equal(o["tag_logp"][:, 0], p["tag_logp"]) and np.array_equal(o["score"][:, 0], p["score"])
        assert np.array_equal(o["masks"][:, 0], p["masks"]) and o["changed"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["tiny_g2w2", "mid_g4w2", "eos_g3w1", "c65"])
def test_without_a_penalty_every_group_is_the_plain_search(name, dtype):
    """Every group selects what the plain search selects, and its values agree to rounding: the eager oracle's products give a row
    other last bits at another place among other rows, in float32 even between two groups of one run.  The rule itself is exact:
    test_the_rule_is_exact_on_given_rows."""
    d, Gd, Wg, o = _oracle(name, 0.0, dtype)
    p = _plain(name, Wg, dtype)
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    assert o["changed"] == 0
    for j in range(Gd):
        assert np.array_equal(o["templates"][:, j], p["templates"])
        np.testing.assert_allclose(o["tag_logp"][:, j], p["tag_logp"], atol=tol)
        np.testing.assert_allclose(o["score"][:, j], p["score"], atol=d.L * tol)
        tr = o["trace"][:, :, j * Wg:(j + 1) * Wg].copy()
        tr[..., 1] -= j * Wg
        assert np.array_equal(tr, p["trace"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_rule_is_exact_on_given_rows(dtype):
    """Steps 3-5 on the same log-probabilities: one group at any lambda, and every group at lambda = 0, ARE the plain merge."""
    rng = np.random.default_rng(5)
    for trial in range(60):
        Gd, Wg = [(1, 3), (2, 2), (4, 2), (3, 1), (2, 4), (1, 8)][trial % 6]
        lam = (0.0, 0.7, 1000.0)[trial % 3] if Gd == 1 else 0.0
        V, L = int(rng.integers(Gd * Wg, 40)), 7
        pair, plain = pdo.PairSearch(Gd, Wg, L, dtype, lam), pbo.VideoSearch(Wg, L, dtype)
        for t in range(L):
            lp = (rng.integers(-6, 0, (Wg, V)) * 0.5 + rng.random((Wg, V)) * (trial % 2)).astype(dtype)
            lp[:, 1] -= dtype(1000)
            par, tok = pair.feed(np.tile(lp, (Gd, 1)))
            q, c = plain.feed(lp)
            assert np.array_equal(par.reshape(Gd, Wg) - np.arange(Gd)[:, None] * Wg, np.tile(q, (Gd, 1)))
            assert np.array_equal(tok.reshape(Gd, Wg), np.tile(c, (Gd, 1)))
        want = plain.result()
        for got in pair.result():
            for g, w in zip(got, want):
                assert np.array_equal(g["seq"], w["seq"]) and np.array_equal(g["logps"], w["logps"]) and g["score"] == w["score"]
                assert (g["t"], g["slot"]) == (w["t"], w["slot"])
        assert pair.changed == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", list(pdo.CASES))
def test_a_large_penalty_keeps_the_live_tags_of_the_groups_apart(name, dtype):
    if name == "c1_g2w3" and dtype == torch.float32:
        dtype = torch.float64                                     # (the real layer sizes once)
    d, Gd, Wg, o = _oracle(name, 1000.0, dtype)
    assert o["disjoint"]
    pdo.trace_in_range(o["trace"], C=d.C, L=d.L, Gd=Gd, Wg=Wg)
    # the unpenalised log-probabilities are what is returned: their sum is the score less the penalties, a multiple of 1000
    # (a beam that continues a finished one starts from -1000 instead of its tags' sum: only live scores are sums of a whole path)
    pen = (o["tag_logp"].astype(np.float64).sum(3) - o["score"])[o["score"] > pbo.LIVE]
    assert pen.size and (np.abs(pen - 1000 * np.round(pen / 1000)) < 1e-2).all()


# ---- the top-N lemma: a row's Wg best penalised values lie inside its unpenalised top N
def _top_n_rows(lp, N):
    """The rows with everything outside their top N (beam_before order) at -3000."""
    ix = np.argsort(-lp, axis=1, kind="stable")[:, :N]
    out = np.full_like(lp, -3000)
    np.put_along_axis(out, ix, np.take_along_axis(lp, ix, 1), 1)
    return out


def test_top_n_rows_give_the_selection_of_the_full_rows():
    rng = np.random.default_rng(11)
    steps = 0
    for trial in range(200):
        Gd, Wg = [(2, 2), (2, 3), (4, 2), (8, 1), (3, 2), (2, 4), (1, 5), (3, 1)][trial % 8]
        N = Gd * Wg
        V = int(rng.integers(N, 62))
        lam = (0.0, 0.5, 1000.0)[trial % 3]
        L = 8
        full, top = pdo.PairSearch(Gd, Wg, L, np.float32, lam), pdo.PairSearch(Gd, Wg, L, np.float32, lam)
        for t in range(L):
            lp = (rng.integers(-6, 0, (N, V)) * 0.5).astype(np.float32)       # tie-heavy: eleven values
            lp[:, 0] -= np.float32(2.0 if t < 3 else 0.0)                     # ends come late: dead slots from step 3 on
            lp[:, 1] -= np.float32(1000)                                      # a suppressed word
            a, b = full.feed(lp.copy()), top.feed(_top_n_rows(lp, N))
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (trial, t)
            steps += 1
        assert np.array_equal(full.trace, top.trace)
        if lam == 1000.0:
            assert full.disjoint
    assert steps == 1600


# ---- the preconditions of the GPU cases (tests/test_gpu_pos_diverse.py), as counts on the float64 oracle at lambda = 0.5 / 1000:
# (group steps whose selection the penalty changes, dead slots whose tag a later live slot takes, videos whose groups finish at
# different steps, videos with a float64 margin >= 1e-3)
PRE = {
    "tiny_g2w2": ((30, 0, 0, 5), (30, 0, 5, 5)),
    "tiny_g3w1": ((35, 0, 0, 5), (60, 0, 0, 5)),
    "tiny_g5w1": ((83, 0, 0, 5), (115, 0, 5, 5)),
    "a_r_odd": ((15, 0, 3, 3), (18, 0, 3, 3)),
    "mid_g2w4": ((80, 0, 0, 3), (96, 0, 0, 5)),
    "mid_g4w2": ((179, 0, 0, 7), (278, 0, 0, 8)),
    "mid_g8w1": ((587, 0, 0, 6), (664, 0, 0, 5)),
    "eos_g2w2": ((24, 0, 8, 7), (27, 0, 8, 8)),
    "eos_g3w1": ((16, 2, 8, 7), (17, 2, 8, 7)),
    "eos_g4w2": ((143, 0, 8, 2), (185, 8, 8, 3)),
    "c64": ((5, 0, 0, 2), (12, 0, 0, 2)),
    "c65": ((12, 0, 0, 1), (12, 0, 0, 1)),
    "c130": ((5, 0, 0, 1), (24, 0, 0, 1)),
    "c1_g2w3": ((182, 0, 0, 4), (203, 0, 0, 3)),
}


def counts(o, B):
    apart = sum(1 for r in o["finish"] if len({tuple(g) for g in r}) > 1)
    return o["changed"], o["dead_reused"], apart, int((o["margin"] >= pbo.MARGIN).sum())


@pytest.mark.parametrize("name", list(pdo.CASES))
def test_gpu_case_preconditions(name):
    assert set(PRE) == set(pdo.CASES)
    dd, _, _, Gd, Wg = pdo.CASES[name][:5]
    assert 1 <= Gd * Wg <= min(8, dd["C"]) and 4 * Gd * Wg * (2 * dd["R"] + dd["C"]) + 1536 <= 65536
    for lam, want in zip((pdo.LAMBDA, 1000.0), PRE[name]):
        d, _, _, o = _oracle(name, lam)
        assert counts(o, d.B) == want, (name, lam, counts(o, d.B))
        assert want[0] >= 1 and want[3] >= 1                      # the penalty changes a selection; a margin pins a video
        assert o["near_dead"] > 400                               # no live sum comes near -500
    # over the cases: groups that finish at different steps, a dead slot's tag taken by a later live slot, N = C, both head forms
    assert PRE["eos_g3w1"][0][1] >= 1 and PRE["eos_g4w2"][1][1] >= 1 and PRE["eos_g2w2"][0][2] >= 1
    assert pdo.CASES["tiny_g5w1"][3] == pdo.CASES["tiny_g5w1"][0]["C"]
    assert [pdo.CASES[k][0]["C"] for k in ("c64", "c65", "c130")] == [64, 65, 130]


def test_admissibility_check_accepts_the_oracle_and_refuses_a_wrong_search():
    d, P, run, x, Gd, Wg = pdo.case("eos_g3w1")
    _, _, _, o = _oracle("eos_g3w1", pdo.LAMBDA, torch.float32)
    lp = pbo.logps_along_trace(po.to_torch(P, torch.float64), po.to_torch(run, torch.float64), *_inputs(x, torch.float64), o["trace"])
    kw = dict(L=d.L, Gd=Gd, Wg=Wg, suppress=1)
    n, live = pdo.check_admissible_groups(o["trace"], o["tag_logp"], o["score"], o["templates"], lp, lam=pdo.LAMBDA, **kw)
    assert n >= d.B * Gd and live.shape == (d.B, d.L, Gd * Wg)
    with pytest.raises(AssertionError):                           # the same search judged under another penalty
        pdo.check_admissible_groups(o["trace"], o["tag_logp"], o["score"], o["templates"], lp, lam=0.0, **kw)
    with pytest.raises(AssertionError):                           # penalised log-probabilities returned
        pdo.check_admissible_groups(o["trace"], o["tag_logp"] - 0.5 * (o["tag_logp"] != 0), o["score"], o["templates"], lp,
                                    lam=pdo.LAMBDA, **kw)
    _, _, _, o3 = _oracle("eos_g3w1", 1000.0, torch.float32)
    lp3 = pbo.logps_along_trace(po.to_torch(P, torch.float64), po.to_torch(run, torch.float64), *_inputs(x, torch.float64), o3["trace"])
    _, live3 = pdo.check_admissible_groups(o3["trace"], o3["tag_logp"], o3["score"], o3["templates"], lp3, lam=1000.0, **kw)
    assert pdo.live_tokens_disjoint(o3["trace"], live3, Gd=Gd, Wg=Wg) >= d.B
    _, _, _, o0 = _oracle("eos_g3w1", 0.0, torch.float32)
    lp0 = pbo.logps_along_trace(po.to_torch(P, torch.float64), po.to_torch(run, torch.float64), *_inputs(x, torch.float64), o0["trace"])
    _, live0 = pdo.check_admissible_groups(o0["trace"], o0["tag_logp"], o0["score"], o0["templates"], lp0, lam=0.0, **kw)
    with pytest.raises(AssertionError):                           # without a penalty the groups share every live tag
        pdo.live_tokens_disjoint(o0["trace"], live0, Gd=Gd, Wg=Wg)


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_pos_beam_diverse.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgpd_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgpd_beam_templates", "xgpd_version", "xgpd_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgpd_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_pos_beam_diverse.h":
            assert not re.search(r"xgpd_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_and_sizes_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_beam as npb
    from controllable_xgating_amd import _native_pos_beam_diverse as npd
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_pos_beam_diverse.h"\nint main(void) {\n'
                   '  printf("%zu %d %d %d %d %zu %d\\n", sizeof(XgpDims), XGPD_VERSION, XGPB_VERSION, XGPD_MAX_BEAM, XGPB_MAX_BEAM, '
                   'XGPD_LDS_BYTES(8, 512, 20), XGPD_MAX_LDS_BYTES);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, ver, bver, nmax, wmax, lds, ldsmax = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                             text=True).stdout.split())
    L = npd.lib()
    assert ver == npd.XGPD_VERSION == L.xgpd_version() == 1 and bver == npb.XGPB_VERSION
    assert nmax == wmax == npd.XGPD_MAX_BEAM == 8 and lds == 4 * 8 * (2 * 512 + 20) + 1536 and ldsmax == 64 * 1024
    assert sd == ctypes.sizeof(npos.XgpDims)


def _mk(d, **kw):
    from controllable_xgating_amd import _native_pos as npos
    v = dict(d._asdict(), **kw)
    return npos.XgpDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["C"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native_pos_beam as npb
    from controllable_xgating_amd import _native_pos_beam_diverse as npd
    L, Lb = npd.lib(), npb.lib()
    B = ctypes.byref
    d = po.make_dims(**po.POS_CFG["mid"])                          # C = 20
    dims = _mk(d)
    size = lambda Gd, Wg, dm=dims: L.xgpd_workspace_bytes(B(dm), Gd, Wg)       # noqa: E731
    for W in range(1, 9):                                          # one group: the plain search's workspace
        assert size(1, W) == Lb.xgpb_workspace_bytes(B(dims), W) > 0
    # the same N in more groups: only done_n grows, by one int32 per video and extra group (the carver rounds its regions up)
    for Gd, Wg in ((2, 4), (4, 2), (8, 1)):
        assert 0 <= size(Gd, Wg) - size(1, 8) <= 4 * d.B * (Gd - 1) + 64
    for Gd, Wg in ((0, 2), (2, 0), (-1, 2), (2, -1), (3, 3), (9, 1), (1, 9), (2, 5), (1 << 16, 1 << 16), (1 << 30, 2)):
        assert size(Gd, Wg) == 0, (Gd, Wg)
    c5 = _mk(d, C=5)
    assert size(5, 1, c5) > 0 and size(1, 5, c5) > 0 and size(2, 3, c5) == 0 and size(3, 2, c5) == 0      # N > C
    assert size(2, 2, _mk(d, B=0)) == 0 and size(2, 2, _mk(d, L=0)) == 0 and L.xgpd_workspace_bytes(None, 2, 2) == 0
    # the merge workgroup's LDS at W = N: 4 N (2 R + C) + 1536 <= 65536
    fits, over = _mk(d, R=990), _mk(d, R=991)
    assert 4 * 8 * (2 * 990 + 20) + 1536 <= 65536 < 4 * 8 * (2 * 991 + 20) + 1536
    assert size(2, 4, fits) > 0 and size(4, 2, over) == 0 and size(7, 1, over) > 0


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_beam_diverse as npd
    L = npd.lib()
    d = po.make_dims(**po.POS_CFG["mid"])                          # C = 20
    B = ctypes.byref
    dims = _mk(d)
    need = L.xgpd_workspace_bytes(B(dims), 2, 2)
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def call(dm=dims, Gd=2, Wg=2, lam=0.5, sup=1, p=P, b=bn, ptrs=None, ws=fake, nbytes=big):
        a = [fake] * 9 if ptrs is None else ptrs       # fr, fo, fm, templates, tag_logp, score, masks, n_out, trace
        return L.xgpd_beam_templates(None, B(dm), Gd, Wg, lam, sup, None if p is None else B(p), None if b is None else B(b), a[0],
                                     a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=need - 1) == -4
    assert call(Gd=4, nbytes=need) == -4 and call(Wg=3, nbytes=need) == -4      # the workspace of (2, 2) serves neither
    assert call(Gd=1, Wg=1, nbytes=8) == -4 and call(Gd=8, Wg=1, nbytes=8) == -4 and call(Gd=1, Wg=8, nbytes=8) == -4
    assert call(lam=0.0, nbytes=8) == -4 and call(lam=1000.0, nbytes=8) == -4 and call(lam=3e38, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=19, nbytes=8) == -4
    # XG_EINVAL: the groups, ahead of the workspace's size
    for Gd, Wg in ((0, 2), (2, 0), (-1, 2), (2, -3), (3, 3), (9, 1), (1, 9), (1 << 16, 1 << 16)):
        assert call(Gd=Gd, Wg=Wg, nbytes=8) == -1, (Gd, Wg)
    c5 = _mk(d, C=5)
    assert call(dm=c5, Gd=5, Wg=1, nbytes=8) == -4 and call(dm=c5, Gd=2, Wg=3, nbytes=8) == -1        # N > C
    # ... the penalty
    for lam in (-0.5, -1e-30, float("inf"), float("-inf"), float("nan")):
        assert call(lam=lam, nbytes=8) == -1, lam
    assert call(lam=-0.0, nbytes=8) == -4
    # ... and what the plain search refuses
    assert call(sup=20, nbytes=8) == -1 and call(dm=c5, sup=5, nbytes=8) == -1
    assert call(dm=_mk(d, B=0)) == -1 and call(dm=_mk(d, L=0)) == -1
    assert call(dm=_mk(d, R=991), Gd=4, Wg=2) == -1 and call(dm=_mk(d, R=991), Gd=7, Wg=1, nbytes=8) == -4
    assert call(p=None) == -1 and call(b=None) == -1 and call(ws=None) == -1
    for i in range(8):
        ptrs = [fake] * 9
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1, i
    ptrs = [fake] * 9
    ptrs[8] = None                                                            # trace may be NULL: the next check decides
    assert call(ptrs=ptrs, nbytes=8) == -4


# ---- the Python surface
def test_train_mode_cpu_tensors_and_bad_arguments_raise(built):
    from controllable_xgating_amd import XgError
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])                         # C = 5
    m = PosModel(pco.make_opt(d))                                  # a fresh module is in train mode
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    with pytest.raises(NotImplementedError):
        m.beam_templates_diverse(*f, 2, 2)
    m.eval()
    # the search's own checks come behind the mode's gate and ahead of the device's
    for Gd, Wg in ((0, 2), (2, 0), (-1, -1), (2, 3), (3, 2), (6, 1), (1, 6), (9, 1)):
        with pytest.raises(ValueError, match="groups"):
            m.beam_templates_diverse(*f, Gd, Wg)
    for lam in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="diversity"):
            m.beam_templates_diverse(*f, 2, 2, diversity=lam)
    with pytest.raises(ValueError, match="suppress_tag"):
        m.beam_templates_diverse(*f, 2, 2, suppress_tag=5)
    with pytest.raises(XgError):                                   # CPU tensors: refused, nothing falls back
        m.beam_templates_diverse(*f, 2, 2)


class _StubPos:
    def __init__(self, B, L):
        self.B, self.L, self.calls = B, L, []

    def beam_templates_diverse(self, fr, fo, fm, groups, group_size, diversity=0.5, suppress_tag=1, trim=True, return_trace=False):
        self.calls.append((fr, fo, fm, groups, group_size, diversity, suppress_tag, trim, return_trace))
        tm = torch.zeros(self.B, groups, group_size, self.L, dtype=torch.int64)
        tm[:, 1:, :, 0] = 2                                        # group 0 differs from the others, which repeat one another
        tm[:, :, 1:, 1] = 3
        score = -torch.arange(self.B * groups * group_size, dtype=torch.float32).reshape(self.B, groups, group_size)
        return tm, torch.zeros(tm.shape), score, torch.ones(self.B, groups, group_size, self.L + 1)

    def sample_forced(self, fr, fo, fm, templates, collect_states=False, trim=False):
        B, S, L = templates.shape
        self.forced = templates
        return torch.full((B, S, L), -0.5), None, None, torch.zeros(B * S, 6)


class _StubCap:
    def sample(self, fr, fo, fm, pos, opt={}):
        self.rows = fr.shape[0]
        return torch.ones(fr.shape[0], 4, dtype=torch.int64), torch.zeros(fr.shape[0], 4)


def test_caption_beam_diverse_flattens_the_groups_and_marks_first_occurrences():
    import controllable_xgating_amd as pkg
    from controllable_xgating_amd import caption_beam_diverse
    assert "caption_beam_diverse" in pkg.__all__ and "diverse_beam_captions_with_templates" in pkg.__all__
    B, L, K, Gd, Wg = 3, 5, 2, 3, 2
    fr, fo, fm = torch.rand(B, K, 7), torch.rand(B, K, 3), torch.ones(B, K)
    pm, cap = _StubPos(B, L), _StubCap()
    seq, slp, tm, score, first = caption_beam_diverse(pm, cap, fr, fo, fm, Gd, Wg, diversity=0.25, suppress_tag=-1)
    (a, b, c, g, w, lam, sup, trim, tr), = pm.calls
    assert a is fr and b is fo and c is fm and (g, w, lam, sup, trim, tr) == (Gd, Wg, 0.25, -1, False, False)
    N = Gd * Wg
    assert tm.shape == (B, N, L) and score.shape == (B, N) and first.shape == (B, N) and first.dtype == torch.bool
    assert pm.forced.shape == (B, N, L) and torch.equal(pm.forced, tm) and cap.rows == B * N
    assert seq.shape[:2] == (B, N) and slp.shape == seq.shape
    assert torch.equal(score[0], -torch.arange(N, dtype=torch.float32))       # template g * Wg + k is the k-th best of group g
    assert first[0].tolist() == [True, True, True, True, False, False]        # group 2 repeats group 1
    with pytest.raises(NotImplementedError, match="beam_captions_with_templates"):
        caption_beam_diverse(pm, cap, fr, fo, fm, Gd, Wg, opt={"beam_size": 5}, share_encoder=True)
    assert len(pm.calls) == 1
    caption_beam_diverse(pm, cap, fr, fo, fm, Gd, Wg)
    assert pm.calls[1][5:7] == (0.5, 1)                            # the defaults of beam_templates_diverse
