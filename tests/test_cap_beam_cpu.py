"""CPU checks of the captioner's beam search: the beam oracle (tests/cap_beam_oracle.py) against the reference's fixtures
tests/golden/cap_beam_*.npz, its ranking and tie rules on hand-built cases; the C ABI of include/xgate_beam.h (exports, version,
error codes without a GPU); and the refusals of SAModel.beam_captions.  No compute on a GPU."""
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
from tests import pos_beam_oracle as pbo
from tests import util
from tests.util import ROOT

FIXTURES = tuple(cbo.BEAM_CASES)


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


@functools.lru_cache(maxsize=None)
def _oracle(name):
    d, P, x, W, g = cbo.load_case(name)
    torch.set_num_threads(8)
    return d, W, g, cbo.beam_captions(P, x, d.L, W)


# ---- the oracle against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_consistent_with_steps_3_to_5(name):
    """The replay of the reference's own W + 1 largest log-probabilities reproduces the tokens it fed, its returned beams are the
    first W completions, and the stored done list and margins are that replay's."""
    d, _, _, W, g = cbo.load_case(name)
    assert g["top_lp"].shape == g["top_ix"].shape == (d.B, d.L, W, W + 1) and g["tokens"].shape == (d.B, d.L, W)
    assert (g["top_lp"][..., :-1] >= g["top_lp"][..., 1:]).all() and g["top_ix"].min() >= 0 and g["top_ix"].max() < d.V
    for b, vs in enumerate(cbo.replay_fixture(g, W, d.L)):
        assert np.array_equal(vs.trace[:, :, 0], g["tokens"][b])
        n = int(g["done_n"][b])
        assert n == len(vs.done) >= W
        assert [(e["t"], e["slot"]) for e in vs.done] == list(zip(g["done_t"][b, :n], g["done_slot"][b, :n]))
        assert np.array_equal(np.array([e["score"] for e in vs.done], np.float32), g["done_score"][b, :n])
        for k in range(W):
            assert np.array_equal(vs.done[k]["seq"], g["ref_seq"][b, k]) and np.array_equal(vs.done[k]["logps"], g["ref_logps"][b, k])
        assert vs.margin == g["margin"][b]


def test_fixture_margins_are_the_documented_ones():
    pinned = {n: int((cbo.load_case(n)[4]["margin"] >= cbo.MARGIN).sum()) for n in FIXTURES}
    assert pinned["tiny_w3"] == 4 and pinned["eos_w3"] == 4 and pinned["c1_w5"] == 0 and pinned["mideos_w5"] >= 1
    g = cbo.load_case("eos_w3")[4]
    assert ((g["done_t"] >= 0) & (g["done_t"] < 5)).sum(1).tolist() == [1, 7, 1, 2, 2]              # early completions (L = 6)
    g = cbo.load_case("mideos_w5")[4]
    assert (((g["done_t"] >= 0) & (g["done_t"] < 6)).sum(1) >= 13).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_logps_along_the_recorded_search(name):
    """Teacher-forced along the reference's own parents and tokens, the oracle's log-probabilities are the reference's at 2e-5
    wherever the reference's were recorded."""
    d, P, x, W, g = cbo.load_case(name)
    trace = np.array([vs.trace for vs in cbo.replay_fixture(g, W, d.L)])
    lp = cbo.logps_along_trace(P, x, trace, torch.float32)
    assert lp.shape == (d.B, d.L, W, d.V)
    lp[..., 1] -= np.float32(1000)
    np.testing.assert_allclose(np.take_along_axis(lp, g["top_ix"], 3), g["top_lp"], atol=2e-5)
    # ... and nothing outside the recorded W + 1 lies above the last of them by more than that
    rest = lp.copy()
    np.put_along_axis(rest, g["top_ix"], -np.inf, 3)
    assert (rest.max(3) <= g["top_lp"][..., -1] + 2e-5).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_tokens_and_completions_where_the_margin_allows(name):
    d, W, g, o = _oracle(name)
    ok = np.flatnonzero(g["margin"] >= cbo.MARGIN)
    for b in ok:
        assert np.array_equal(o["tokens"][b], g["tokens"][b]), b
        assert np.array_equal(o["top_ix"][b, :, :, :W], g["top_ix"][b, :, :, :W]), b
        np.testing.assert_allclose(o["top_lp"][b], g["top_lp"][b], atol=2e-5)
        for k in range(W):                                        # the reference's returned beams: the first W completions
            assert np.array_equal(o["done"][b][k]["seq"], g["ref_seq"][b, k]), (b, k)
            np.testing.assert_allclose(o["done"][b][k]["logps"], g["ref_logps"][b, k], atol=2e-5)
        n = int(g["done_n"][b])
        assert [(e["t"], e["slot"]) for e in o["done"][b]] == list(zip(g["done_t"][b, :n], g["done_slot"][b, :n]))
    # whatever the margins: the shape of the result
    sq, lp = o["seq"], o["seq_logp"]
    assert sq.shape == (d.B, W, d.L) and lp.shape == sq.shape and o["score"].shape == (d.B, W)
    assert (o["score"][:, :-1] >= o["score"][:, 1:]).all()
    for b in range(d.B):
        for k, e in enumerate(o["ranked"][b]):
            assert (sq[b, k, e["t"] + 1:] == 0).all() and (lp[b, k, e["t"] + 1:] == 0).all()
            assert abs(float(lp[b, k].astype(np.float64).sum()) - float(e["score"])) < 1e-3 or e["score"] < cbo.LIVE


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_and_float64_oracles_return_the_same_beams(name):
    d, P, x, W, g = cbo.load_case(name)
    o32, o64 = _oracle(name)[3], cbo.beam_captions(P, x, d.L, W, dtype=torch.float64)
    assert np.array_equal(o32["seq"], o64["seq"])
    np.testing.assert_allclose(o32["seq_logp"], o64["seq_logp"], atol=2e-5)


def test_best_beam_is_the_existing_host_fixture():
    """The oracle's best beam at W = 3 is tests/golden/beam_tiny.npz and beam_c1.npz (the reference's own sample(beam_size=3))."""
    for tag in ("tiny", "c1"):
        gb = util.load_golden("beam_%s.npz" % tag)
        c = dict(util.CFG[tag])
        c["B"] = min(c["B"], 3)
        d = pg.make_dims(**c)
        o = cbo.beam_captions(pg.make_params(d), pg.make_inputs(d, seed=0), d.L, int(gb["beam_size"]))
        assert np.array_equal(o["seq"][:, 0], gb["seq"]), tag
        np.testing.assert_allclose(o["seq_logp"][:, 0], gb["seqLogprobs"], atol=2e-5)


def test_ranking_uses_the_score_at_the_finish():
    """The best beam is not the first to finish: a hand-built search through the fixtures' sparse-row replay."""
    W, L = 2, 3
    ln = lambda *p: np.log(np.array(p, np.float32))               # noqa: E731
    rows = lambda *r: cbo.sparse_rows(np.stack([v for v, _ in r]), np.stack([np.array(i) for _, i in r]))     # noqa: E731
    vs = pbo.VideoSearch(W, L, np.float32)
    # step 0: word 7 (log .8) and word 0 (log .1): slot 1 finishes first, with the lower score
    vs.feed(rows((ln(0.8, 0.1, 0.05), [7, 0, 3]), (ln(0.8, 0.1, 0.05), [7, 0, 3])))
    assert [(e["t"], e["slot"]) for e in vs.done] == [(0, 1)]
    # step 1: [7, 0] finishes second with log .72 > log .1
    vs.feed(rows((ln(0.9, 0.05, 0.01), [0, 9, 4]), (ln(0.4, 0.3, 0.2), [5, 6, 8])))
    assert [(e["t"], e["slot"]) for e in vs.done] == [(0, 1), (1, 0)]
    vs.feed(rows((ln(0.5, 0.3, 0.1), [2, 3, 4]), (ln(0.5, 0.3, 0.1), [2, 3, 4])))
    res = vs.result()
    assert res[0]["seq"].tolist() == [7, 0, 0] and res[1]["seq"].tolist() == [0, 0, 0]
    np.testing.assert_allclose([res[0]["score"], res[1]["score"]], np.log([0.72, 0.1]), atol=1e-6)
    assert res[0]["logps"][2] == 0 and res[1]["logps"][1] == 0
    # the eos fixtures' beams finish at different steps
    d, W, g, o = _oracle("eos_w3")
    assert len({e["t"] for b in range(d.B) for e in o["done"][b]}) > 2


def _flat_head(P):
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.full_like(P["logit.bias"], 0.25)
    return P


# what the tie rule gives when every word is as likely as every other, W = 3, steps 0 and 1: (token, parent) per slot
TIE_TRACE = {1: [[(0, 0), (2, 0), (3, 0)], [(0, 1), (0, 2), (2, 1)]],        # word 1 suppressed
             -1: [[(0, 0), (1, 0), (2, 0)], [(0, 1), (0, 2), (1, 1)]]}


@pytest.mark.parametrize("suppress", [1, -1])
def test_all_equal_logits_follow_the_tie_rule(suppress):
    d = pg.make_dims(**dict(util.CFG["tiny"], B=2))
    P, x = _flat_head(pg.make_params(d)), pg.make_inputs(d, seed=3)
    o = cbo.beam_captions(P, x, d.L, 3, suppress_token=suppress)
    for b in range(d.B):
        assert [[tuple(v) for v in step] for step in o["trace"][b, :2].tolist()] == TIE_TRACE[suppress]
    assert (o["seq"][:, 0] == 0).all()                                       # the first completion is the empty caption, log(1 / V)
    np.testing.assert_allclose(o["score"][:, 0], -np.log(d.V), atol=1e-5)
    if suppress == 1:
        assert not ((o["seq"] == 1) & (o["seq_logp"] > cbo.LIVE)).any()
    else:
        assert (o["seq"] == 1).any()


# ---- the C ABI
def _beam_header():
    txt = open(os.path.join(ROOT, "include", "xgate_beam.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgcb_[a-z_0-9]+)\s*\(", _beam_header())))
    assert syms == ["xgcb_beam_search", "xgcb_version", "xgcb_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgcb_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_beam.h":
            assert not re.search(r"xgcb_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_and_constants_through_gcc(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam as nb
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_beam.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(XgDims), sizeof(XgBnState), sizeof(XgBatch), sizeof(XgRun), '
                   'XGCB_VERSION, XG_VERSION, XGCB_MAX_BEAM);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sb, sx, sr, ver, xver, wmax = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    L = nb.lib()
    assert ver == nb.XGCB_VERSION == L.xgcb_version() == 1
    assert xver == nv.XG_VERSION == 206 and wmax == nb.XGCB_MAX_BEAM == 8
    assert (sd, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgBnState, nv.XgBatch, nv.XgRun))


def test_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam as nb
    L = nb.lib()
    d = pg.make_dims(**util.CFG["mid"])                            # V = 500
    B = ctypes.byref

    def mk(**kw):
        v = dict(d._asdict(), **kw)
        return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)

    dims = mk()
    sizes = [L.xgcb_workspace_bytes(B(dims), W) for W in range(1, 9)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))      # grows with W
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

    def call(dm=dims, W=3, sup=1, p=P, b=bn, x=None, r=None, outs=None, ws=fake, nbytes=big):
        o = [fake] * 4 if outs is None else outs       # seq, seq_logp, score, trace
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgcb_beam_search(None, B(dm), W, sup, None if p is None else B(p), None if b is None else B(b),
                                  None if x is False else B(x), None if r is False else B(r), o[0], o[1], o[2], o[3], ws, nbytes)

    # every pointer set (never dereferenced: the checks run first), but the workspace too small -> XG_EWORKSPACE
    assert call(nbytes=8) == -4 and call(nbytes=sizes[2] - 1) == -4
    assert call(W=4, nbytes=sizes[2]) == -4                                    # the workspace of W = 3 does not serve W = 4
    assert call(W=1, nbytes=8) == -4 and call(W=8, nbytes=8) == -4
    assert call(sup=-1, nbytes=8) == -4 and call(sup=-7, nbytes=8) == -4 and call(sup=0, nbytes=8) == -4 and call(sup=499, nbytes=8) == -4
    # XG_EINVAL, and no workspace size
    for W in (0, -1, 9, 64):
        assert call(W=W) == -1 and L.xgcb_workspace_bytes(B(dims), W) == 0, W
    v5 = mk(V=5)
    assert call(dm=v5, W=5, nbytes=8) == -4 and call(dm=v5, W=6) == -1 and L.xgcb_workspace_bytes(B(v5), 6) == 0      # W > V
    assert call(sup=500) == -1 and call(sup=1 << 20) == -1 and call(dm=v5, sup=5) == -1
    bad, one = mk(B=0), mk(L=0)                                               # a search needs T >= 2
    assert call(dm=bad) == -1 and call(dm=one) == -1
    assert L.xgcb_workspace_bytes(B(bad), 3) == 0 and L.xgcb_workspace_bytes(B(one), 3) == 0 and L.xgcb_workspace_bytes(None, 3) == 0
    assert L.xgcb_workspace_bytes(B(mk(B=1 << 20)), 8) == 0                   # too many rows
    assert call(r=run(train=1)) == -1 and call(r=run(save=1)) == -1
    assert call(r=run(gemm_mode=1)) == -1 and call(r=run(gemm_mode=3)) == -1
    assert call(p=None) == -1 and call(b=None) == -1 and call(x=False) == -1 and call(r=False) == -1 and call(ws=None) == -1
    assert call(ws=fake + 16) == -1                                           # the workspace is 256-byte aligned
    assert call(b=nv.XgBnState(fake, fake, None, fake)) == -1
    for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"):
        assert call(x=batch(**{k: None})) == -1, k
    for i in range(3):
        outs = [fake] * 4
        outs[i] = None
        assert call(outs=outs) == -1, i
    assert call(outs=[fake, fake, fake, None], nbytes=8) == -4                # trace may be NULL: the next check decides


# ---- the Python surface
def test_train_mode_cpu_tensors_and_bad_widths_raise(built):
    d = pg.make_dims(**util.CFG["tiny"])
    m = util.make_model(d, device="cpu", train=True)
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"])
    with pytest.raises(NotImplementedError):
        m.beam_captions(*f, beam_size=3)
    m.eval()
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.beam_captions(*f, beam_size=3)
    with pytest.raises(NotImplementedError):
        m.sample(*f, {"beam_size": 3, "beam_on_device": True})
    for W in (0, 9, d.V + 1):
        with pytest.raises(ValueError):
            m.beam_captions(*f, beam_size=W)
    with pytest.raises(ValueError):
        m.beam_captions(*f, beam_size=3, suppress_token=d.V)
    m.precision = "bf16"
    with pytest.raises(NotImplementedError):
        m.beam_captions(*f, beam_size=3)
