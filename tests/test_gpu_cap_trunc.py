"""Truncated (top-k / nucleus) caption sampling on the MI355X: SAModel.sample_truncated_per_video (include/xgate_truncate.h,
csrc/xg_heads.hip: rollout_trunc_kernel) against the float64 oracle of tests/cap_trunc_oracle.py, which implements
docs/CAPTION_TRUNCATED.md; then the exact consequences of the definition, ties, determinism and workspace independence, and
control.caption_truncated_with_templates.

Bounds: the project's own for this model.  Tokens are equal row by row; a row may differ only when its first difference (token
or kept count) is excused on the oracle's float64 quantities -- the uniform within 3e-4 of an edge of the token's interval of
the truncated CDF, or the kept set itself on an edge: the threshold class within the 1e-3 logit margin of the next value below
it, or a cumulative mass at the threshold (with or without the threshold class) within 3e-4, relative, of top_p Z_k.  At most 2
rows per case may differ: tests/test_cap_trunc_cpu.py shows on the CPU that the oracle in float32 against itself in float64
stays within that cap (it measures 0 rows) for every (case, setting) run here.  Before a row's first difference kept is exact
and both log-probabilities are within 3e-4."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_trunc_oracle as co
from tests.util import assert_sampled_tokens_match, make_model

pytestmark = pytest.mark.gpu
LP_TOL = 3e-4
CDF_TOL = 3e-4
MASS_TOL = 3e-4
MARGIN = 1e-3
MAX_ROWS = 2
THREADS = 1024                                                  # rollout_trunc_kernel's workgroup
STAGE_BYTES = 150 * 1024                                        # a row of at most this many bytes is staged in LDS
SMALL = ["tiny_s5", "mid_b3_s5", "odd_s2", "peaked"]
IDS = ["%s-T%g-k%d-p%g" % ((n,) + s) for n, s in co.PAIRS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def test_cases_reach_the_branches_they_name():
    c = {k: v[0] for k, v in co.CASES.items()}
    rows = {k: v[0]["B"] * v[1] for k, v in co.CASES.items()}
    tile_stats = lambda d, m: m <= 128 and d["R"] % 32 == 0 and d["V"] >= 32                       # noqa: E731 (xgk_vocab_select_ok)
    t = c["tiny_s5"]
    assert t["V"] == 61 < THREADS and not tile_stats(t, rows["tiny_s5"]) and t["E"] % 4            # the generic step, xgk_linear
    m = c["mid_b3_s5"]
    assert m["V"] == 500 and tile_stats(m, rows["mid_b3_s5"]) and m["V"] < 4096                    # 32-column statistics
    assert m["R"] % 32 == 0 and m["E"] % 4 == 0 and m["A"] % 4 == 0                                # the packed step
    assert c["odd_s2"]["V"] == 37 and c["odd_s2"]["V"] % 4
    r = c["c1_s8"]
    assert r["V"] == 20000 and r["V"] * 4 <= STAGE_BYTES and tile_stats(r, rows["c1_s8"]) and r["V"] >= 4096
    assert r["V"] > 19 * THREADS                                                                   # 20 columns per thread
    assert rows["rows_297"] == 297 > 256 and not tile_stats(c["rows_297"], 297)                    # logits from xgk_linear
    assert c["big_v"]["V"] * 4 > STAGE_BYTES and 24 * THREADS < c["big_v"]["V"] <= 64 * THREADS    # not staged; two load rounds
    assert c["huge_v"]["V"] > 64 * THREADS                                                         # columns behind the search's bit set
    assert c["peaked"] == m and co.CASES["peaked"][2] > 1.0
    # every setting runs on some case with V above and below the thread count, and the two searches run alone and together
    assert {(k > 1, p < 1) for _, k, p in co.SETTINGS} == {(False, True), (True, False), (True, True), (False, False)}
    assert any(k == 1 for _, k, _ in co.SETTINGS)


# ---- the device side (models and inputs once per case)
@functools.lru_cache(maxsize=None)
def _model(name):
    d, _, P = co.inputs(name)[:3]
    return make_model(d, P, train=False)


@functools.lru_cache(maxsize=None)
def _dev(name):
    d, S, _, x, pos, u = co.inputs(name)
    f = tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    return f, torch.from_numpy(pos).cuda().reshape(d.B, S, d.R), torch.from_numpy(u).cuda()


def _run(name, setting, model=None, uniforms=None, stats=True, trim=True):
    """-> numpy (seq (M,n), seq_logp, seq_logq, kept[, n]), rows flattened"""
    d, S = co.inputs(name)[:2]
    f, pos, u = _dev(name)
    T, k, p = setting
    out = (model or _model(name)).sample_truncated_per_video(*f, pos, top_k=k, top_p=p, temperature=T,
                                                             uniforms=u if uniforms is None else uniforms, return_stats=stats, trim=trim)
    torch.cuda.synchronize()
    assert all(not o.requires_grad for o in out) and out[0].dtype == torch.int64 and out[0].shape[:2] == (d.B, S)
    if stats:
        assert out[3].dtype == torch.int32 and out[2].dtype == torch.float32
    res = [o.cpu().numpy() for o in out]
    return [a.reshape(d.B * S, -1) if a.ndim == 3 else a for a in res]


def _live(seq):
    """(M,n) bool: the steps up to and including a row's end token"""
    return np.concatenate([np.ones((seq.shape[0], 1), bool), seq[:, :-1] > 0], 1)


def _pad(a, n):
    return np.concatenate([a, np.zeros((a.shape[0], n - a.shape[1]), a.dtype)], 1)


def _excused(o, u, setting, b, k, token_differs):
    """Is a difference of row b at column k excused by the oracle's float64 quantities of that draw?  -> (bool, what was measured)"""
    T, top_k, top_p = setting
    tok, _, _, _, K, (lo, hi) = co.draw(o["logits"][k][b], u[k + 1, b], T, top_k, top_p)
    uu = float(u[k + 1, b])
    edge = min(abs(uu - lo), abs(uu - hi))
    gap = K.thr - K.below
    mass = min(abs(K.mass_at - K.need), abs(K.mass_above - K.need)) / K.need if top_p < 1.0 else np.inf
    ok = (token_differs and edge <= CDF_TOL) or gap < MARGIN or mass <= MASS_TOL
    return ok, dict(row=b, col=k, oracle_token=tok, cdf_edge=edge, threshold_gap=gap, mass_rel=mass)


# ---- 1. against the oracle
@pytest.mark.parametrize("name,setting", co.PAIRS, ids=IDS)
def test_against_the_float64_oracle(name, setting):
    d, S, _, _, _, u = co.inputs(name)
    M = d.B * S
    o = co.oracle(name, setting)
    seq, slp, slq, kept = _run(name, setting)
    assert seq.shape == slp.shape == slq.shape == kept.shape and seq.min() >= 0 and seq.max() < d.V
    assert np.isfinite(slp).all() and np.isfinite(slq).all()
    n = max(seq.shape[1], o["n"])
    seq, slp, slq, kept = (_pad(a, n) for a in (seq, slp, slq, kept))
    seq_o, slp_o, slq_o, kept_o = (_pad(o[k], n) for k in ("seq", "seq_logp", "seq_logq", "kept"))
    live = _live(seq_o)
    differ, worst = [], [0.0, 0.0]
    for b in range(M):
        ne = np.flatnonzero((seq[b] != seq_o[b]) | (kept[b] != kept_o[b]))
        stop = int(ne[0]) if ne.size else n
        if ne.size:
            ok, what = _excused(o, u, setting, b, stop, seq[b, stop] != seq_o[b, stop])
            assert ok, what
            differ.append(what)
        lv = live[b, :stop]
        assert np.array_equal(kept[b, :stop], kept_o[b, :stop])
        for i, (a, ref) in enumerate(((slp, slp_o), (slq, slq_o))):
            err = np.abs(a[b, :stop][lv] - ref[b, :stop][lv])
            if err.size:
                worst[i] = max(worst[i], float(err.max()))
        assert (slq[b, :stop][~lv] == 0).all() and (kept[b, :stop][~lv] == 0).all()
    kl = kept_o[live]
    print("%s %s: %d of %d rows differ %s; max |dlogp| %.2e, |dlogq| %.2e; kept %d .. %d (mean %.1f) of %d; n = %d"
          % (name, setting, len(differ), M, differ, worst[0], worst[1], kl.min(), kl.max(), kl.mean(), d.V, o["n"]))
    assert worst[0] <= LP_TOL and worst[1] <= LP_TOL, worst
    assert len(differ) <= MAX_ROWS, differ
    if not differ:
        assert _run(name, setting)[0].shape[1] == o["n"]


# ---- 2. exact consequences of the definition
@pytest.mark.parametrize("name", SMALL)
def test_top_k_1_is_the_greedy_rollout_for_any_uniforms(name):
    d, S = co.inputs(name)[:2]
    f, pos, u = _dev(name)
    g, glp = _model(name).sample_per_video(*f, pos, {"sample_max": 1})
    g, glp = g.cpu().numpy().reshape(d.B * S, -1), glp.cpu().numpy().reshape(d.B * S, -1)
    for uu, T, p in ((u, 1.0, 1.0), (1.0 - u, 0.6, 0.4), (torch.zeros_like(u), 1.0, 1.0)):
        seq, slp, slq, kept = _run(name, (T, 1, p), uniforms=uu)
        assert np.array_equal(seq, g)
        live = _live(seq)
        assert (kept[live] == 1).all() and (kept[~live] == 0).all() and (slq == 0).all()
        assert np.abs(slp - glp)[live].max() <= 1e-5


@pytest.mark.parametrize("name,temperature", [("tiny_s5", 1.0), ("mid_b3_s5", 0.7), ("odd_s2", 1.3), ("peaked", 1.0)])
def test_both_off_is_the_plain_sampled_rollout(name, temperature):
    d, S, _, _, _, u = co.inputs(name)
    f, pos, ud = _dev(name)
    seq, slp, slq, kept = _run(name, (temperature, 0, 1.0))
    ps, plp = _model(name).sample_per_video(*f, pos, {"sample_max": 0, "temperature": temperature, "uniforms": ud})
    ps, plp = ps.cpu().numpy().reshape(d.B * S, -1), plp.cpu().numpy().reshape(d.B * S, -1)
    live = _live(seq)
    assert (kept[live] == d.V).all() and (kept[~live] == 0).all()
    # the two kernels group the sums differently (by thread chunk / by tile): equal up to the CDF-edge rule, each against the oracle
    o = co.oracle(name, (temperature, 0, 1.0))
    logps = [torch.log_softmax(torch.from_numpy(x), 1) for x in o["logits"]]
    rows = set(assert_sampled_tokens_match(seq, o["seq"], logps, u, temperature, tol=CDF_TOL))
    rows |= set(assert_sampled_tokens_match(ps, o["seq"], logps, u, temperature, tol=CDF_TOL))
    diff = co.first_differences(seq, ps)
    assert set(diff) <= rows and len(diff) <= MAX_ROWS, (diff, rows)
    n = min(seq.shape[1], ps.shape[1])
    same = [b for b in range(d.B * S) if b not in diff]
    assert np.abs(slp[same, :n] - plp[same, :n])[live[same, :n]].max() <= 1e-5
    if temperature == 1.0:                                         # nothing truncated, nothing tempered: q is p
        assert np.abs(slq - slp)[live].max() <= 1e-5


@pytest.mark.parametrize("name", SMALL)
def test_log_probabilities_and_kept_counts_obey_the_definition(name):
    d, S = co.inputs(name)[:2]
    V = d.V
    for setting in co.SETTINGS + [(1.0, 3, 1.0), (1.0, V, 0.7), (1.0, V + 7, 1.0)]:
        T, k, p = setting
        seq, slp, slq, kept = _run(name, setting)
        live = _live(seq)
        assert (slq <= 0).all() and (slq[kept == 1] == 0).all() and (slq[~live] == 0).all() and (kept[~live] == 0).all()
        assert (kept[live] >= 1).all() and (kept[live] <= V).all()
        if T == 1.0:
            # q renormalises p over a subset: log q >= log p, up to the float32 rounding of two sums of V terms grouped differently
            assert (slq - slp)[live].min() >= -1e-5
        kk = min(k, V) if k > 0 else V
        if p == 1.0:
            assert (kept[live] >= kk).all()
            ties = kept[live] != kk                                # seeded float weights: no two words share a logit
            assert not ties.any()
        else:
            assert (kept[live] <= kk).all()
    # the first draw reads the same logits whatever the setting: adding top_p to top_k can only shrink its kept set
    k_only, both = _run(name, (0.7, 8, 1.0))[3][:, 0], _run(name, (0.7, 8, 0.8))[3][:, 0]
    assert (both <= k_only).all() and (both >= 1).all()


# ---- 3. ties are kept
def test_ties_at_the_threshold_are_kept_and_drawn_in_column_order():
    name = "mid_b3_s5"
    d, S, P, _, _, u0 = co.inputs(name)
    P = dict(P)
    P["logit.weight"], P["logit.bias"] = P["logit.weight"].copy(), P["logit.bias"].copy()
    P["logit.weight"][1::2] = P["logit.weight"][0::2]             # word 2i + 1 := word 2i: paired logits are bit-equal
    P["logit.bias"][1::2] = P["logit.bias"][0::2]
    assert d.V % 2 == 0
    m = make_model(d, P, train=False)
    u = np.where(u0 < 0.5, u0 * 0.98, 0.51 + (u0 - 0.5) * 0.98).astype(np.float32)    # away from 0.5
    assert (np.abs(u - 0.5) >= 0.01 - 1e-6).all() and (u < 1).all() and (u >= 0).all()
    ud = torch.from_numpy(u).cuda()
    seq, slp, slq, kept = _run(name, (1.0, 1, 1.0), model=m, uniforms=ud)
    live = _live(seq)
    assert live.sum() > d.B * S and (kept[live] == 2).all()
    uu = u[1:seq.shape[1] + 1].T                                   # the uniform of column c is uniforms[c + 1]
    assert ((seq % 2 == 1) == (uu > 0.5))[live].all()              # the even word below one half, the odd one above
    assert np.abs(slq[live] - np.log(0.5)).max() <= 1e-6
    g = m.sample_per_video(*_dev(name)[0], _dev(name)[1], {"sample_max": 1})[0].cpu().numpy().reshape(d.B * S, -1)
    first = np.flatnonzero(uu[:, 0] < 0.5)                         # (rows that took the even word at the first draw took the argmax)
    assert first.size and np.array_equal(seq[first, 0], g[first, 0])
    kept3 = _run(name, (1.0, 3, 1.0), model=m, uniforms=ud)
    assert (kept3[3][_live(kept3[0])] == 4).all()
    kept2 = _run(name, (1.0, 2, 1.0), model=m, uniforms=ud)
    assert (kept2[3][_live(kept2[0])] == 2).all()


# ---- 4. determinism and the workspace
@pytest.mark.parametrize("name", SMALL)
def test_result_is_deterministic_and_does_not_depend_on_the_workspace(name):
    from tests import ws_state as wss
    m = _model(name)
    setting = (0.7, 8, 0.8)

    def both():
        return _run(name, setting, trim=False) + _run(name, (1.0, 0, 0.9), trim=False)

    first, again = both(), both()
    # the workspace the calls above used, every 32-bit word a quiet NaN (the words a kernel waits on included: every call
    # zeroes them before its first launch, as the rollout over rows per video does), and a larger block than asked for
    (key, ws), = m._control_ws.items()
    dirty_ws = torch.empty(ws.numel() + 4096, dtype=torch.uint8, device=ws.device)
    dirty_ws[:ws.numel()] = ws
    dirty_ws.view(torch.int32).fill_(wss.NAN32)
    m._control_ws = {key: dirty_ws}
    dirty = both()
    for a, b_, c in zip(first, again, dirty):
        assert np.isfinite(a).all()
        assert np.array_equal(a, b_) and np.array_equal(a, c)      # bit for bit: no float atomics anywhere in the draw
    d, S = co.inputs(name)[:2]
    assert first[0].shape == (d.B * S, d.L) and 1 <= int(first[4][0]) <= d.L and (first[0][:, int(first[4][0]):] == 0).all()
    # return_stats=False hands the library null pointers for seq_logq and kept
    out = _run(name, setting, stats=False, trim=False)
    assert len(out) == 3 and np.array_equal(out[0], first[0]) and np.array_equal(out[1], first[1]) and np.array_equal(out[2], first[4])
    # without uniforms the draws come from torch's generator on the device
    g = torch.Generator(device="cuda")
    f, pos, _ = _dev(name)
    a = m.sample_truncated_per_video(*f, pos, top_k=8, generator=g.manual_seed(5), trim=False)[0]
    b_ = m.sample_truncated_per_video(*f, pos, top_k=8, generator=g.manual_seed(5), trim=False)[0]
    c = m.sample_truncated_per_video(*f, pos, top_k=8, generator=g.manual_seed(6), trim=False)[0]
    assert torch.equal(a, b_) and not torch.equal(a, c)


# ---- 5. through the chain, and the raises
def test_caption_truncated_with_templates_is_the_two_call_chain():
    from controllable_xgating_amd import caption_truncated_with_templates
    from tests import pos_control_oracle as pco
    from tests import pos_oracle as po
    from tests.util import CFG
    dp = po.make_dims(**po.POS_CFG["tiny"])
    dc = pg.make_dims(**CFG["tiny"])
    assert (dp.B, dp.K, dp.R, dp.F1, dp.F2) == (dc.B, dc.K, dc.R, dc.F1, dc.F2)
    S = 3
    pm = pco.pos_model(dp, po.make_params(dp), po.make_running(dp))
    tm, _ = pco.seeded_templates(dp.B, S, dp.L, dp.C, seed=11)
    fr, fo, fm = pco.cuda_inputs(po.make_inputs(dp, seed=20, ragged=True))
    cap = make_model(dc, pg.make_params(dc), train=False)
    u = torch.from_numpy(pg.uniform("u", (dc.L + 1, dc.B * S), 7)).cuda()
    kw = dict(top_k=9, top_p=0.85, temperature=0.8, uniforms=u)
    seq, slp, score, slq, kept = caption_truncated_with_templates(pm, cap, fr, fo, fm, tm, return_stats=True, **kw)
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
        want = cap.sample_truncated_per_video(fr, fo, fm, pos_feats.reshape(dc.B, S, -1), return_stats=True, **kw)
    assert torch.equal(score, tag_logp.sum(2)) and score.shape == (dc.B, S)
    for a, b_ in zip((seq, slp, slq, kept), want):
        assert torch.equal(a, b_) and not a.requires_grad
    assert int(kept.max()) <= 9 and int(kept.min()) >= 0 and seq.shape[:2] == (dc.B, S)
    three = caption_truncated_with_templates(pm, cap, fr, fo, fm, tm, **kw)
    assert len(three) == 3 and torch.equal(three[0], seq) and torch.equal(three[1], slp) and torch.equal(three[2], score)
    # the plain one-row-per-video case is pos_feats (B,1,R)
    one = cap.sample_truncated_per_video(fr, fo, fm, pos_feats.reshape(dc.B, S, -1)[:, :1].contiguous(), top_k=4,
                                         uniforms=u[:, :dc.B].contiguous(), return_stats=True)
    assert one[0].shape[:2] == (dc.B, 1) and int(one[3].max()) == 4
    # the raises of the method and the wrapper
    pos = pos_feats.reshape(dc.B, S, -1)
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.01), dict(temperature=0.0), dict(uniforms=u[:-1]),
                dict(uniforms=u.cpu()), dict(uniforms=u[:, :-1])):
        with pytest.raises(ValueError):
            cap.sample_truncated_per_video(fr, fo, fm, pos, **bad)
        with pytest.raises(ValueError):
            caption_truncated_with_templates(pm, cap, fr, fo, fm, tm, **bad)
    for bad in (pos.reshape(dc.B * S, -1), pos[:-1], pos[:, :, :-1]):
        with pytest.raises(ValueError):
            cap.sample_truncated_per_video(fr, fo, fm, bad)
    with pytest.raises(NotImplementedError):
        cap.sample_truncated_per_video(fr.cpu(), fo, fm, pos)
    cap.precision = "bf16"
    with pytest.raises(NotImplementedError):
        caption_truncated_with_templates(pm, cap, fr, fo, fm, tm, **kw)
    cap.precision = "fp32"
    cap.train()
    with pytest.raises(NotImplementedError):
        cap.sample_truncated_per_video(fr, fo, fm, pos, **kw)
    cap.eval()
    again = cap.sample_truncated_per_video(fr, fo, fm, pos, return_stats=True, **kw)      # ... and it still runs after the refusals
    assert all(torch.equal(a, b_) for a, b_ in zip(again, want))
