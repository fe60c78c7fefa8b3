"""Scoring given captions on the MI355X: SAModel.score_captions_per_video (include/xgate_score.h) against the float64 replay of
oracle.xgate_oracle on the batch with every video repeated per row (tests/cap_score_oracle.py), over every branch of the scoring
kernels (csrc/xg_score.hip), of the chunking and of the step forms around them; then cross mode row by row, determinism, workspace
independence, the old replay, the beam search's own log-probabilities, and control.score_captions_with_templates.

Bounds: LP_TOL = 3e-4 on every counted tok_logp (the project's bound for this model; the float32 oracle itself deviates by 4e-7 at
the default gain), count * LP_TOL on score, count exact, uncounted columns exactly 0, no row excused.  The cases, their captions and
what they reach: tests/cap_score_oracle.py, checked without a GPU in tests/test_cap_score_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_score_oracle as cso
from tests.cap_score_oracle import LP_TOL
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
CASES = cso.cases()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def test_cases_reach_the_branches_they_name():
    import re
    from controllable_xgating_amd import _native_control as ncc
    from tests.util import ROOT
    G = ncc.XGCC_TEMPLATE_GROUP
    src = open(ROOT + "/controllable_xgating_amd/csrc/xg_kernels.h").read() + open(ROOT + "/controllable_xgating_amd/csrc/xg_model.hip").read()
    assert int(re.search(r"XGK_SCORE_TILE\s*=\s*(\d+)", src).group(1)) == cso.TILE          # the ONE tile width: 32 columns
    assert int(re.search(r"SC_CHUNK\s*=\s*(\d+)", src).group(1)) == cso.CHUNK
    c = {k: v[0] for k, v in CASES.items()}
    q = {k: v[1] for k, v in CASES.items()}
    fast = lambda d: d["R"] % 32 == 0 and d["V"] >= cso.TILE      # noqa: E731  (xg_score.hip: score_fast; operands are aligned)
    packed = lambda d: d["R"] % 8 == 0 and d["E"] % 4 == 0 and d["A"] % 4 == 0      # noqa: E731  (xg_model.hip: step_packed)
    assert c["tiny_q3"]["B"] * q["tiny_q3"] == 15 and q["tiny_q3"] < G
    assert q["tiny_q5"] == G + 1 and q["tiny_q9"] == 2 * G + 1                                # partial attention groups
    m = c["mid_b3_q5"]
    assert packed(m) and fast(m) and m["V"] == 500 and m["V"] % cso.TILE == 20 and m["B"] * q["mid_b3_q5"] == 15
    assert m["L"] == 2 * cso.CHUNK + 1                               # two whole chunks and one of a single step; the ring wraps once
    o = c["odd_q2"]
    assert o["R"] % 8 and not packed(o) and not fast(o) and o["V"] == 37 and o["L"] == cso.CHUNK + 1
    assert c["one_q3"]["K"] == 1 and c["one_q3"]["L"] == 1 and c["one_q3"]["V"] == 5 and not fast(c["one_q3"])
    assert c["rows_297"]["B"] * q["rows_297"] == 297 and not fast(c["rows_297"])
    r = c["rows_297_r32"]
    assert r["B"] * q["rows_297_r32"] == 297 and fast(r) and 2 * cso.ROW_TILE < 297 < 3 * cso.ROW_TILE
    assert (cso.CHUNK * 297) % cso.ROW_TILE                            # ... and a chunk's 891 rows end in a partial row tile too
    r = c["c1_q8"]
    assert fast(r) and packed(r) and (r["V"], r["R"], r["E"], r["A"]) == (20000, 512, 468, 1536) and r["L"] % cso.CHUNK == 2
    assert fast(c["mid_v4100"]) and c["mid_v4100"]["V"] == 128 * cso.TILE + 4
    assert fast(c["hot"]) and CASES["hot"][2] == 512.0 and (c["hot"]["B"], q["hot"]) == (3, 2)


# ---- the model and the device inputs of a case (made once, shared, never changed)
@functools.lru_cache(maxsize=None)
def _model(name):
    d, _, P = cso.case_inputs(name)[:3]
    return make_model(d, P, train=False)


@functools.lru_cache(maxsize=None)
def _dev(name):
    d, Q, _, x, pos, tokens = cso.case_inputs(name)
    f = tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    return f, torch.from_numpy(pos).cuda().reshape(d.B, Q, d.R), torch.from_numpy(tokens).cuda().reshape(d.B, Q, d.L)


def _score(name, **kw):
    f, pos, cap = _dev(name)
    out = _model(name).score_captions_per_video(*f, pos, cap, **kw)
    torch.cuda.synchronize()
    assert all(not t.requires_grad for t in out)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.float32 and out[2].dtype == torch.int32
    return [t.cpu().numpy() for t in out]


def _check(got, ref, tokens, tol=LP_TOL, what=""):
    """(tok_logp, score, count) as (M,L), (M), (M) against the oracle's: every counted column within tol, every other exactly 0,
    count exact, score within count * tol.  Prints the figures before it asserts."""
    lp, sc, cnt = got
    lp_o, sc_o, cnt_o = ref
    counted = cso.counted_columns(tokens)
    err = np.abs(lp - lp_o)[counted].max()
    serr = (np.abs(sc - sc_o) / cnt_o).max()
    print("%s: max |tok_logp - oracle| %.3e (bound %.1e), max |score - oracle| / count %.3e" % (what, err, tol, serr))
    assert np.isfinite(lp).all() and np.isfinite(sc).all()
    assert np.array_equal(cnt, cnt_o)
    assert (lp[~counted] == 0).all()
    assert err <= tol
    assert (np.abs(sc - sc_o) <= cnt_o * tol).all()


# ---- 2. every case against the float64 oracle
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_replay(name):
    d, Q, _, _, _, tokens = cso.case_inputs(name)
    M = d.B * Q
    lp, sc, cnt = _score(name)
    assert lp.shape == (d.B, Q, d.L) and sc.shape == (d.B, Q) and cnt.shape == (d.B, Q)
    _check((lp.reshape(M, d.L), sc.reshape(M), cnt.reshape(M)), cso.case_reference(name), tokens, what=name)


# ---- 3. cross mode: every caption under every template, placed row by row
def test_cross_mode_places_rows_by_template_then_caption():
    dd = dict(CFG["tiny"], B=2)
    d = pg.make_dims(**dd)
    S, N, seed = 3, 2, 71
    P = pg.make_params(d._replace(B=1))
    x = pg.make_inputs(d, seed=seed, ragged=True)
    pos = pg.uniform("pos_cross", (d.B, S, d.R), seed, -1.0, 1.0)
    cap = cso.edge_captions(3, d.L, d.V, seed)[1:].reshape(1, N, d.L).repeat(d.B, 0)          # a full caption and one with a late EOS
    cap[1, :, 0] = [7, 9]
    m = make_model(d, P, train=False)
    f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
    lp, sc, cnt = m.score_captions_per_video(*f, torch.from_numpy(pos).cuda(), torch.from_numpy(cap).cuda(), cross=True)
    torch.cuda.synchronize()
    assert lp.shape == (d.B, S, N, d.L) and sc.shape == (d.B, S, N) and cnt.shape == (d.B, S, N)
    # the oracle over the rows (b, s, n): template s, caption n
    pos_rows = np.repeat(pos, N, 1).reshape(d.B * S * N, d.R)
    tok_rows = np.tile(cap[:, None], (1, S, 1, 1)).reshape(d.B * S * N, d.L)
    ref = cso.score_rows(P, x, pos_rows, tok_rows, S * N)
    _check((lp.cpu().numpy().reshape(-1, d.L), sc.cpu().numpy().reshape(-1), cnt.cpu().numpy().reshape(-1)), ref, tok_rows, what="cross")
    # placement would show: rows of one video are apart by far more than the bound, along s and along n
    r = ref[0].reshape(d.B, S, N, d.L)
    assert np.abs(r[:, 0] - r[:, 1]).max() > 100 * LP_TOL and np.abs(r[:, :, 0] - r[:, :, 1]).max() > 100 * LP_TOL
    # ... and cross = False on the same rows handed over explicitly gives the same bits
    lp2, sc2, cnt2 = m.score_captions_per_video(*f, torch.from_numpy(pos_rows).cuda().reshape(d.B, S * N, d.R),
                                                torch.from_numpy(tok_rows).cuda().reshape(d.B, S * N, d.L))
    assert torch.equal(lp2.reshape(lp.shape), lp) and torch.equal(sc2.reshape(sc.shape), sc) and torch.equal(cnt2.reshape(cnt.shape), cnt)
    # a short caption tensor is padded with zeros
    lp3, sc3, cnt3 = m.score_captions_per_video(*f, torch.from_numpy(pos).cuda(), torch.from_numpy(cap[:, :, :2]).cuda().int(), cross=True)
    short = np.concatenate([tok_rows[:, :2], np.zeros((tok_rows.shape[0], d.L - 2), np.int64)], 1)
    _check((lp3.cpu().numpy().reshape(-1, d.L), sc3.cpu().numpy().reshape(-1), cnt3.cpu().numpy().reshape(-1)),
           cso.score_rows(P, x, pos_rows, short, S * N), short, what="cross, L' = 2")
    assert int(cnt3.max()) == 3


# ---- 4. determinism and workspace independence
# Bit for bit at tiny and mid and at the real layer sizes with 64 videos.  With FEW videos at the real layer sizes the encoder's
# embedding products run split-K with atomic adds, for every entry point (tests/test_gpu_cap_control.py has the measurement), so
# c1_q8 gets the suite's bound for two runs of the same call; a NaN or a stale workspace value still fails it.
DET_ONLY = {"c1_b64_q2": (dict(CFG["c1"], B=64, L=4), 2)}


@functools.lru_cache(maxsize=None)
def _det_inputs(name):
    if name in CASES:
        d = cso.case_inputs(name)[0]
        return (d, _model(name)) + _dev(name)
    dd, Q = DET_ONLY[name]
    d = pg.make_dims(**dd)
    P = pg.make_params(d._replace(B=1))
    x = pg.make_inputs(d, seed=5, ragged=True)
    f = tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    pos = torch.from_numpy(pg.uniform("pos_det", (d.B, Q, d.R), 5, -1.0, 1.0)).cuda()
    cap = torch.from_numpy(cso.edge_captions(d.B * Q, d.L, d.V, 5)).cuda().reshape(d.B, Q, d.L)
    return d, make_model(d, P, train=False), f, pos, cap


@pytest.mark.parametrize("name,exact", [("tiny_q5", True), ("mid_b3_q5", True), ("rows_297_r32", True), ("c1_b64_q2", True), ("c1_q8", False)])
def test_repeat_is_bit_identical_and_the_workspace_does_not_matter(name, exact):
    d, m, f, pos, cap = _det_inputs(name)

    def once():
        junk = [torch.full(tuple(cap.shape), float("nan"), device="cuda"), torch.full(tuple(cap.shape[:2]), float("nan"), device="cuda"),
                torch.full(tuple(cap.shape[:2]), -1, dtype=torch.int32, device="cuda")]          # what torch.empty hands the outputs next
        del junk
        out = m.score_captions_per_video(*f, pos, cap)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    first, again = once(), once()
    (key, ws), = m._score_ws.items()
    m._score_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}      # NaN bytes, and larger
    dirty = once()
    for a, b_, c in zip(first, again, dirty):
        assert np.isfinite(a).all() and np.isfinite(b_).all() and np.isfinite(c).all()
        if exact or a.dtype != np.float32:
            assert np.array_equal(a, b_) and np.array_equal(a, c)
        else:
            tol = 1e-5 * np.abs(a).max() + 1e-8
            assert np.abs(a - b_).max() <= tol and np.abs(a - c).max() <= tol, (np.abs(a - b_).max(), np.abs(a - c).max(), tol)
    assert (first[2] >= 1).all() and (first[2] <= d.L).all()


def test_without_side_streams_the_result_is_the_same(monkeypatch):
    """XgRun.aux == NULL puts the chunks on the caller's stream; the arithmetic does not know."""
    name = "mid_b3_q5"
    with_aux = _score(name)
    with monkeypatch.context() as mp:
        mp.setattr(_model(name), "_aux_handle", lambda: None)
        plain = _score(name)
    for a, b_ in zip(with_aux, plain):
        assert np.array_equal(a, b_)


# ---- 5. against the old replay and the beam search
def test_counted_columns_agree_with_sample_forced_tokens():
    name = "tiny_q5"
    d, Q, _, _, _, tokens = cso.case_inputs(name)
    M = d.B * Q
    f, pos, cap = _dev(name)
    with torch.no_grad():
        _, slp, _ = _model(name).sample(*[t.repeat_interleave(Q, 0) for t in f], pos.reshape(M, d.R),
                                        {"forced_tokens": cap.reshape(M, d.L), "async": True})
    lp = _score(name)[0].reshape(M, d.L)
    counted = cso.counted_columns(tokens)
    err = np.abs(lp - slp.cpu().numpy())[counted].max()
    print("against sample(forced_tokens): max difference in the counted columns %.3e" % err)
    assert err <= 2 * LP_TOL


def test_rescoring_the_beam_search_reproduces_its_log_probabilities():
    name, W = "mid_b3_q5", 3
    d, S = cso.case_inputs(name)[:2]
    f, pos, _ = _dev(name)
    m = _model(name)
    seq, seq_logp, score = m.beam_captions_per_video(*f, pos, beam_size=W, suppress_token=-1)
    rows = pos.unsqueeze(2).expand(d.B, S, W, d.R).reshape(d.B, S * W, d.R)
    lp, sc, cnt = m.score_captions_per_video(*f, rows, seq.reshape(d.B, S * W, d.L))
    torch.cuda.synchronize()
    lp, sc, cnt = lp.cpu().numpy().reshape(-1, d.L), sc.cpu().numpy().reshape(-1), cnt.cpu().numpy().reshape(-1)
    tok = seq.cpu().numpy().reshape(-1, d.L)
    counted = cso.counted_columns(tok)
    err = np.abs(lp - seq_logp.cpu().numpy().reshape(-1, d.L))[counted].max()
    print("against the beam search: max |tok_logp - seq_logp| %.3e, max |score difference| / count %.3e"
          % (err, (np.abs(sc - score.cpu().numpy().reshape(-1)) / cnt).max()))
    assert np.array_equal(cnt, counted.sum(1)) and (lp[~counted] == 0).all()
    assert (seq_logp.cpu().numpy().reshape(-1, d.L)[~counted] == 0).all()            # the beam's own zeros: its steps ARE the counted columns
    assert err <= 2 * LP_TOL
    assert (np.abs(sc - score.cpu().numpy().reshape(-1)) <= cnt * 2 * LP_TOL).all()


# ---- 6. through control.py
def test_score_captions_with_templates_is_its_two_parts():
    from controllable_xgating_amd import score_captions_with_templates, template_recovery
    from tests import pos_control_oracle as pco
    from tests import pos_oracle as po
    dp = po.make_dims(**po.POS_CFG["tiny"])
    dc = pg.make_dims(**CFG["tiny"])
    assert (dp.B, dp.K, dp.R, dp.F1, dp.F2) == (dc.B, dc.K, dc.R, dc.F1, dc.F2)
    S = 3
    pm = pco.pos_model(dp, po.make_params(dp), po.make_running(dp))
    tm, _ = pco.seeded_templates(dp.B, S, dp.L, dp.C, seed=11)
    fr, fo, fm = pco.cuda_inputs(po.make_inputs(dp, seed=20, ragged=True))
    cap_model = make_model(dc, pg.make_params(dc), train=False)
    cap = torch.from_numpy(cso.edge_captions(dc.B * S, dc.L, dc.V, 9)).cuda().reshape(dc.B, S, dc.L)
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
    for cross in (False, True):
        got = score_captions_with_templates(pm, cap_model, fr, fo, fm, tm, cap, cross=cross)
        parts = cap_model.score_captions_per_video(fr, fo, fm, pos_feats.reshape(dc.B, S, -1), cap, cross=cross)
        assert len(got) == 4 and all(not t.requires_grad for t in got)
        assert all(torch.equal(a, b_) for a, b_ in zip(got[:3], parts)) and torch.equal(got[3], tag_logp.sum(2))
        assert got[3].shape == (dc.B, S) and got[1].shape == ((dc.B, S, S) if cross else (dc.B, S))
    rec = template_recovery(got[1])
    assert rec.shape == (dc.B, S) and rec.dtype == torch.bool and rec.is_cuda
    sc = got[1].cpu().numpy()
    assert np.array_equal(rec.cpu().numpy(), np.stack([[sc[b, s, s] >= sc[b, :, s].max() for s in range(S)] for b in range(dc.B)]))
