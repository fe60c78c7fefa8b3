"""CPU checks of POS beam search: the beam oracle (tests/pos_beam_oracle.py) against the reference's fixtures
tests/golden/pos_beam_*.npz, its ranking and tie rules on hand-built cases; the C ABI of include/xgate_pos_beam.h (exports, version,
struct sizes, error codes without a GPU); and the refusals of PosModel.beam_templates.  No compute on a GPU."""
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
from tests import pos_oracle as po
from tests.util import ROOT

FIXTURES = tuple(pbo.BEAM_CASES)


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def _cpu_inputs(x):
    return [torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask")]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    d, P, run, x, W, g = pbo.load_case(name)
    torch.set_num_threads(8)
    return d, W, g, pbo.beam_templates(po.to_torch(P), po.to_torch(run), *_cpu_inputs(x), d.L, W)


def _replay(g, W):
    """Steps 3-5 over the fixture's own log-probabilities: one VideoSearch per video."""
    B, L = g["tokens"].shape[:2]
    out = []
    for b in range(B):
        vs = pbo.VideoSearch(W, L, np.float32)
        for t in range(L):
            s = g["logps"][b, t].copy()
            s[:, 1] -= np.float32(1000)
            vs.feed(s)
        out.append(vs)
    return out


# ---- the oracle against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_consistent_with_steps_3_to_5(name):
    """The replay of the reference's own log-probabilities reproduces the tokens it fed, its returned beams are the first W
    completions, and the stored done list and margins are that replay's."""
    _, W = pbo.BEAM_CASES[name]
    g = dict(np.load(os.path.join(pbo.GOLD, "pos_beam_%s.npz" % name)))
    for b, vs in enumerate(_replay(g, W)):
        assert np.array_equal(vs.trace[:, :, 0], g["tokens"][b])
        n = int(g["done_n"][b])
        assert n == len(vs.done) >= W
        assert [(e["t"], e["slot"]) for e in vs.done] == list(zip(g["done_t"][b, :n], g["done_slot"][b, :n]))
        assert np.array_equal(np.array([e["score"] for e in vs.done], np.float32), g["done_score"][b, :n])
        for k in range(W):
            assert np.array_equal(vs.done[k]["seq"], g["ref_seq"][b, k]) and np.array_equal(vs.done[k]["logps"], g["ref_logps"][b, k])
        assert vs.margin == g["margin"][b]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_logps_along_the_recorded_search(name):
    """Teacher-forced along the reference's own parents and tokens, the oracle's log-probabilities are the reference's at 2e-5."""
    d, P, run, x, W, g = pbo.load_case(name)
    trace = np.array([vs.trace for vs in _replay(g, W)])
    lp = pbo.logps_along_trace(po.to_torch(P), po.to_torch(run), *_cpu_inputs(x), trace)
    assert lp.shape == g["logps"].shape == (d.B, d.L, W, d.C)
    np.testing.assert_allclose(lp, g["logps"], atol=2e-5)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_tokens_and_completions_where_the_margin_allows(name):
    d, W, g, o = _oracle(name)
    ok = np.flatnonzero(g["margin"] >= pbo.MARGIN)
    if name.startswith("tiny"):
        assert len(ok) == d.B
    if name == "eos_w3":
        assert len(ok) >= 5
    for b in ok:
        assert np.array_equal(o["tokens"][b], g["tokens"][b]), b
        np.testing.assert_allclose(o["logps"][b], g["logps"][b], atol=2e-5)
        for k in range(W):                                        # the reference's returned beams: the first W completions
            assert np.array_equal(o["done"][b][k]["seq"], g["ref_seq"][b, k]), (b, k)
            np.testing.assert_allclose(o["done"][b][k]["logps"], g["ref_logps"][b, k], atol=2e-5)
        n = int(g["done_n"][b])
        assert [(e["t"], e["slot"]) for e in o["done"][b]] == list(zip(g["done_t"][b, :n], g["done_slot"][b, :n]))
    # whatever the margins: the shape of the result
    tm, lp, mk = o["templates"], o["tag_logp"], o["masks"]
    assert tm.shape == (d.B, W, d.L) and lp.shape == tm.shape and mk.shape == (d.B, W, d.L + 1) and o["score"].shape == (d.B, W)
    assert (o["score"][:, :-1] >= o["score"][:, 1:]).all()
    assert (mk[:, :, 0] == 1).all() and np.array_equal(mk, pbo.masks_of(tm))
    for b in range(d.B):
        for k, e in enumerate(o["ranked"][b]):
            assert (tm[b, k, e["t"] + 1:] == 0).all() and (lp[b, k, e["t"] + 1:] == 0).all()
            assert abs(float(lp[b, k].astype(np.float64).sum()) - float(e["score"])) < 1e-3 or e["score"] < pbo.LIVE


def test_tiny_w5_is_the_w_equals_c_case():
    """W = C: the suppressed category sits among the candidates, a video's best beam ends at step 0, and six beams finish."""
    d, W, g, o = _oracle("tiny_w5")
    assert W == d.C and (g["done_n"] == 6).all()
    assert (o["trace"][:, 0, :, 0] == 1).any(1).all()             # category 1 is selected at t = 0: there are only C candidates
    best_at_0 = [b for b in range(d.B) if o["ranked"][b][0]["t"] == 0]
    assert best_at_0
    for b in best_at_0:
        assert (o["templates"][b, 0] == 0).all() and o["masks"][b, 0, 1:].sum() == 0


def test_ranking_uses_the_score_at_the_finish():
    """The best beam is not the first to finish: a hand-built search, and the eos fixtures (their beams finish at different steps)."""
    W, L, C = 2, 3, 4
    vs = pbo.VideoSearch(W, L, np.float32)
    ln = lambda *p: np.log(np.array(p, np.float32))               # noqa: E731
    vs.feed(np.stack([ln(0.1, 0.02, 0.8, 0.08)] * 2))            # slots: tag 2 (p log .8), tag 0 (log .1): slot 1 finishes first
    assert [(e["t"], e["slot"]) for e in vs.done] == [(0, 1)]
    vs.feed(np.stack([ln(0.9, 0.01, 0.05, 0.04), ln(0.25, 0.25, 0.25, 0.25)]))
    assert [(e["t"], e["slot"]) for e in vs.done] == [(0, 1), (1, 0)]     # [2, 0] finishes second with log .72 > log .1
    vs.feed(np.stack([ln(0.25, 0.25, 0.25, 0.25)] * 2))
    res = vs.result()
    assert res[0]["seq"].tolist() == [2, 0, 0] and res[1]["seq"].tolist() == [0, 0, 0]
    np.testing.assert_allclose([res[0]["score"], res[1]["score"]], np.log([0.72, 0.1]), atol=1e-6)
    assert res[0]["logps"][2] == 0 and res[1]["logps"][1] == 0
    # equal scores keep their completion order
    vs = pbo.VideoSearch(2, 1, np.float32)
    vs.feed(np.stack([ln(0.25, 0.25, 0.25, 0.25)] * 2))
    assert [e["slot"] for e in vs.result()] == [0, 1] and vs.trace[0, :, 0].tolist() == [0, 1]
    # the eos fixtures' beams finish at different steps, yet every later completion scores lower: on them (and on every other
    # fixture) the ranking by the score at the finish is the reference's first W completions, so only the hand-built case above
    # tells the two rules apart
    for name in ("eos_w3", "eos_w5"):
        d, W, g, o = _oracle(name)
        assert len({e["t"] for b in range(d.B) for e in o["done"][b]}) > 2
        for b in range(d.B):
            assert all(r is e for r, e in zip(o["ranked"][b], o["done"][b])), (name, b)


def _flat_head(d, P):
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.full_like(P["logit.bias"], 0.25)
    return P


# what the tie rule gives when every category is as likely as every other, W = 3, steps 0 and 1: (token, parent) per slot
TIE_TRACE = {1: [[(0, 0), (2, 0), (3, 0)], [(0, 1), (0, 2), (2, 1)]],        # category 1 suppressed
             -1: [[(0, 0), (1, 0), (2, 0)], [(0, 1), (0, 2), (1, 1)]]}


@pytest.mark.parametrize("suppress", [1, -1])
@pytest.mark.parametrize("Cn", [5, 70])
def test_all_equal_logits_follow_the_tie_rule(Cn, suppress):
    d = po.make_dims(**dict(po.POS_CFG["tiny"], B=2, C=Cn))
    P, run, x = _flat_head(d, po.make_params(d)), po.make_running(d), po.make_inputs(d, seed=3)
    o = pbo.beam_templates(po.to_torch(P), po.to_torch(run), *_cpu_inputs(x), d.L, 3, suppress_tag=suppress)
    for b in range(d.B):
        assert [[tuple(v) for v in step] for step in o["trace"][b, :2].tolist()] == TIE_TRACE[suppress]
    # the first completion is the empty template, with log(1 / C)
    assert (o["templates"][:, 0] == 0).all()
    np.testing.assert_allclose(o["score"][:, 0], -np.log(Cn), atol=1e-5)
    if suppress == 1:
        live = o["tag_logp"] > pbo.LIVE
        assert not ((o["templates"] == 1) & live).any()
    else:
        assert (o["templates"] == 1).any()


# ---- the C ABI
def _beam_header():
    txt = open(os.path.join(ROOT, "include", "xgate_pos_beam.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgpb_[a-z_0-9]+)\s*\(", _beam_header())))
    assert syms == ["xgpb_beam_templates", "xgpb_version", "xgpb_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgpb_[a-z_0-9]+)\b", out))) == syms
    for h in ("xgate_pos.h", "xgate_pos_control.h", "xgate_pos_sample.h", "xgate_pos_train.h", "xgate.h"):
        assert "xgpb_" not in open(os.path.join(ROOT, "include", h)).read(), h


def test_version_and_struct_sizes_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_beam as npb
    from controllable_xgating_amd import _native_pos_control as npc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_pos_beam.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d %d %zu %d\\n", sizeof(XgpDims), sizeof(XgpParams), sizeof(XgBnState), XGPB_VERSION, '
                   'XGPC_VERSION, XGP_VERSION, XGPB_MAX_BEAM, XGPB_LDS_BYTES(8, 512, 20), XGPB_MAX_LDS_BYTES);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, sb, ver, cver, pver, wmax, lds, ldsmax = (
        int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = npb.lib()
    assert ver == npb.XGPB_VERSION == L.xgpb_version() == 1
    assert cver == npc.XGPC_VERSION and pver == npos.XGP_VERSION and wmax == npb.XGPB_MAX_BEAM == 8
    assert lds == 4 * 8 * (2 * 512 + 20) + 1024 and ldsmax == 64 * 1024
    assert sd == ctypes.sizeof(npos.XgpDims) and sp == ctypes.sizeof(npos.XgpParams) and sb == ctypes.sizeof(nv.XgBnState)


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_beam as npb
    from controllable_xgating_amd import _native_pos_control as npc
    L = npb.lib()
    d = po.make_dims(**po.POS_CFG["mid"])                          # C = 20
    B = ctypes.byref

    def mk(**kw):
        v = dict(d._asdict(), **kw)
        return npos.XgpDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["C"], v["F1"], v["F2"], v["L"] + 1)

    dims = mk()
    sizes = [L.xgpb_workspace_bytes(B(dims), W) for W in range(1, 9)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                       # grows with W
    assert all(s > npc.lib().xgpc_workspace_bytes(B(dims), W) > 0 for W, s in zip(range(1, 9), sizes))
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def call(dm=dims, W=3, sup=1, p=P, b=bn, ptrs=None, ws=fake, nbytes=big):
        a = [fake] * 9 if ptrs is None else ptrs       # fr, fo, fm, templates, tag_logp, score, masks, n_out, trace
        return L.xgpb_beam_templates(None, B(dm), W, sup, None if p is None else B(p), None if b is None else B(b), a[0], a[1], a[2],
                                     a[3], a[4], a[5], a[6], a[7], a[8], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=sizes[2] - 1) == -4
    assert call(W=4, nbytes=sizes[2]) == -4                                    # the workspace of W = 3 does not serve W = 4
    assert call(W=1, nbytes=8) == -4 and call(W=8, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=-7, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=19, nbytes=8) == -4
    # XG_EINVAL, and no workspace size
    for W in (0, -1, 9, 64):
        assert call(W=W) == -1 and L.xgpb_workspace_bytes(B(dims), W) == 0, W
    c5 = mk(C=5)
    assert call(dm=c5, W=5, nbytes=8) == -4 and call(dm=c5, W=6) == -1 and L.xgpb_workspace_bytes(B(c5), 6) == 0      # W > C
    assert call(sup=20) == -1 and call(sup=1 << 20) == -1 and call(dm=c5, sup=5) == -1
    bad, one = mk(B=0), mk(L=0)                                               # a search needs T >= 2
    assert call(dm=bad) == -1 and call(dm=one) == -1
    assert L.xgpb_workspace_bytes(B(bad), 3) == 0 and L.xgpb_workspace_bytes(B(one), 3) == 0
    assert L.xgpb_workspace_bytes(B(mk(B=1 << 20)), 8) == 0                   # B * W rows beyond 32-bit offsets
    # the merge workgroup's LDS: 4 W (2 R + C) + 1024 <= 65536
    fits, over = mk(R=998, C=20), mk(R=999, C=20)
    assert 4 * 8 * (2 * 998 + 20) + 1024 <= 65536 < 4 * 8 * (2 * 999 + 20) + 1024
    assert call(dm=fits, W=8, nbytes=8) == -4 and L.xgpb_workspace_bytes(B(fits), 8) > 0
    assert call(dm=over, W=8) == -1 and L.xgpb_workspace_bytes(B(over), 8) == 0
    assert call(dm=over, W=7, nbytes=8) == -4                                 # the same R serves a narrower beam
    assert call(dm=mk(R=4096), W=2) == -1 and call(dm=mk(R=4096), W=1, nbytes=8) == -4
    assert call(p=None) == -1 and call(b=None) == -1 and call(ws=None) == -1
    assert call(p=npos.XgpParams(*([fake] * (len(npos.PARAM_NAMES) - 1) + [None]))) == -1
    for i in range(8):
        ptrs = [fake] * 9
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1, i
    ptrs = [fake] * 9
    ptrs[8] = None                                                            # trace may be NULL: the next check decides
    assert call(ptrs=ptrs, nbytes=8) == -4


# ---- the Python surface
def test_train_mode_cpu_tensors_and_bad_widths_raise(built):
    from controllable_xgating_amd import XgError, caption_beam  # noqa: F401
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(pco.make_opt(d))                           # a fresh module is in train mode
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    with pytest.raises(NotImplementedError):
        m.beam_templates(*f, beam_size=3)
    m.eval()
    with pytest.raises(XgError):
        m.beam_templates(*f, beam_size=3)
    # PosModel.sample keeps refusing a beam: the search has its own entry point
    with pytest.raises(NotImplementedError):
        m.sample(*f, {"beam_size": 3})
