"""The captioner's beam search under decoding rules on the MI355X: SAModel.beam_captions_ruled (include/xgate_beam_rules.h) judged by
tests/cap_rules_oracle.py.  First the kernel's OWN trace replayed in float64 on every case (check_admissible: none excused, the done
list by key) with what the header promises checked exactly -- no live beam holds an n-gram twice, by control.repeated_ngrams on the
device and by a host loop -- against beam_captions_per_video on the same inputs, whose live beams do repeat.  Then bans together
with allowed words, min_length, bad endings, the length-scaled ranking (keys bit for bit), the rules off against
beam_captions_allowed and beam_captions_per_video bit for bit, workspace and trace independence, and
control.beam_captions_ruled_with_templates against its two parts done by hand.

Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4.  Cases and the pinned counts
(counted in float64 on the CPU): tests/cap_rules_oracle.py and tests/test_cap_rules_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_allow_oracle as cao
from tests import cap_rules_oracle as cro
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
LP_TOL, LIVE, MARGIN, ANY = cro.LP_TOL, cro.LIVE, cro.MARGIN, cro.ANY


def _videos(x):
    return tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))


def _flat(out, B, S):
    torch.cuda.synchronize()
    return [v.cpu().numpy().reshape((B * S,) + tuple(v.shape[2:])) for v in out]


def _search(m, x, pos, W, rl=cro.OFF, table=None, masks=None, **kw):
    """beam_captions_ruled, as numpy viewed over the G = B S groups: [seq (G,W,L), seq_logp, score (G,W), key (G,W)[, trace]]."""
    B, S = pos.shape[:2]
    if table is not None:
        kw["word_cat"] = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        kw["allow"] = torch.from_numpy(np.asarray(masks, np.int64)).cuda().reshape(B, S, -1)
    with torch.no_grad():
        out = m.beam_captions_ruled(*_videos(x), torch.from_numpy(pos).cuda(), beam_size=W, no_repeat_ngram=rl["n"],
                                    min_length=rl["min_length"], bad_endings=list(rl["bad_end"]) or None,
                                    length_scale=None if rl["scale"] is None else torch.from_numpy(rl["scale"]), **kw)
    assert out[0].shape[:3] == (B, S, W) and out[2].shape == (B, S, W) and out[3].shape == (B, S, W)
    return _flat(out, B, S)


def _plain(m, x, pos, W, **kw):
    B, S = pos.shape[:2]
    with torch.no_grad():
        out = m.beam_captions_per_video(*_videos(x), torch.from_numpy(pos).cuda(), beam_size=W, **kw)
    return _flat(out, B, S)


@functools.lru_cache(maxsize=None)
def _model(name):
    c = cro.case(name)
    return make_model(c["d"], c["P"], train=False)


@functools.lru_cache(maxsize=None)
def _result(name):
    """A case's search under its rules on the device with its trace, run once and shared: (seq, lp, score, key, trace)."""
    c = cro.case(name)
    return tuple(_search(_model(name), c["x"], c["pos"], c["W"], c["rl"], return_trace=True))


def _finish(seq):
    """(..) the step a returned beam finished at: its first 0, or L - 1."""
    L = seq.shape[-1]
    return np.where((seq == 0).any(-1), (seq == 0).argmax(-1), L - 1)


# ---- 1. the kernel's own trace, judged in float64; no repeated n-gram, exactly; the plain search repeats
@pytest.mark.parametrize("name", cro.TRACE_CASES)
def test_own_trace_is_admissible_and_no_live_beam_repeats(name):
    from controllable_xgating_amd import repeated_ngrams
    c = cro.case(name)
    d, S, W, n = c["d"], c["S"], c["W"], c["rl"]["n"]
    G = d.B * S
    seq, lp, score, key, trace = _result(name)
    assert seq.shape == (G, W, d.L) and seq.dtype == np.int64 and lp.shape == seq.shape and trace.shape == (G, d.L, W, 2)
    assert seq.min() >= 0 and seq.max() < d.V and np.isfinite(score).all() and np.isfinite(lp).all() and np.array_equal(key, score)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, c["rl"]) >= G
    live = score > LIVE
    assert live[:, 0].all()                                      # every group has a live best beam
    rep = repeated_ngrams(torch.from_numpy(seq).cuda(), n).cpu().numpy()
    assert rep.shape == (G, W) and not rep[live].any(), np.argwhere(live & rep)
    for g, k in np.argwhere(live):                               # the same by a host loop
        assert not cro.has_repeat(seq[g, k], n), (g, k, seq[g, k])
    # the same inputs without the rule: live beams repeat (pinned in float64 for the cases whose seed and gain were chosen for it)
    pseq, _, pscore = _plain(_model(name), c["x"], c["pos"], W)
    prep = repeated_ngrams(torch.from_numpy(pseq).cuda(), n).cpu().numpy() & (pscore > LIVE)
    print("%s: plain live beams with a repeated %d-gram: %d of %d" % (name, n, prep.sum(), (pscore > LIVE).sum()))
    if name in cro.REPETITION:
        assert prep.any()                                        # (float64: in every group, PINS)
        assert not np.array_equal(pseq, seq)


# ---- 2. bans together with allowed words
def _allow_setup():
    c = cao.case("tiny_s3w3")
    d = c["d"]
    masks = np.full((d.B * c["S"], d.L), ANY, np.int64)
    return c, d, masks, make_model(d, c["P"], train=False)


def test_pair_category_twice_uses_both_words_once_each():
    c, d, masks, m = _allow_setup()
    S, W = c["S"], c["W"]
    assert W == 3
    masks[0, :2], masks[0, 2:] = 1 << cao.PAIR, 1
    rl = cro.rules(n=1)
    seq, lp, score, key, trace = _search(m, c["x"], c["pos"], W, rl, c["table"], masks, return_trace=True)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, rl, c["table"], masks) >= d.B * S
    pair = sorted(np.flatnonzero(c["table"] == cao.PAIR).tolist())
    live = np.flatnonzero(score[0] > LIVE)
    assert len(live) == 2                                         # "a b" and "b a": the second position leaves each slot one word
    got = sorted(seq[0, k, :3].tolist() for k in live)
    assert got == sorted([[pair[0], pair[1], 0], [pair[1], pair[0], 0]]), got
    assert (seq[0, live, 3:] == 0).all() and np.isfinite(lp).all() and np.isfinite(score).all()


def test_single_category_twice_kills_its_group_and_no_other():
    c, d, masks, m = _allow_setup()
    S, W = c["S"], c["W"]
    rl = cro.rules(n=1)
    base = _search(m, c["x"], c["pos"], W, rl, c["table"], masks, return_trace=True)
    masks2 = masks.copy()
    masks2[1, :2], masks2[1, 2:] = 1 << cao.SINGLE, 1
    seq, lp, score, key, trace = got = _search(m, c["x"], c["pos"], W, rl, c["table"], masks2, return_trace=True)
    assert (score[1] <= LIVE).all() and (key[1] == score[1]).all()
    assert all(np.isfinite(a).all() for a in (lp, score, key)) and seq.min() >= 0 and seq.max() < d.V
    others = [g for g in range(d.B * S) if g != 1]
    for a, b in zip(got, base):                                  # groups never interact
        assert np.array_equal(a[others], b[others])
    assert (score[others, 0] > LIVE).all()
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, rl, c["table"], masks2) >= len(others)


# ---- 3. min_length
@pytest.mark.parametrize("name", ["eos_min3", "eos_min3_n2", "mideos_min3"])
def test_min_length(name):
    c = cro.case(name)
    d, W, mn = c["d"], c["W"], c["rl"]["min_length"]
    G = d.B * c["S"]
    seq, lp, score, key, trace = _result(name)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, c["rl"]) >= G
    live, tf = score > LIVE, _finish(seq)
    assert live[:, 0].all()
    ended = (seq == 0).any(-1)
    assert (tf[live & ended] >= mn).all()                        # a live beam that ends with word 0 has >= min_length words
    early = ended & (tf < mn)                                    # a beam that took word 0 where it was banned: dead, r <= -1000
    assert not (early & live).any()
    assert (np.take_along_axis(lp, tf[..., None], 2)[..., 0][early] <= -1000).all()
    if c["rl"]["n"]:
        assert not any(cro.has_repeat(seq[g, k], c["rl"]["n"]) for g, k in np.argwhere(live))
    pseq, _, pscore = _plain(_model(name), c["x"], c["pos"], W)
    short = [len(cro.words_of(pseq[g, 0])) < mn for g in range(G)]
    print("%s: plain best beams shorter than %d words: %d of %d" % (name, mn, sum(short), G))
    assert sum(short) >= 1                                       # (float64: in every group, PINS)


def test_min_length_of_the_whole_caption():
    c = cro.case("eos_min3")
    d, W = c["d"], c["W"]
    rl = cro.rules(min_length=d.L)
    seq, lp, score, key, trace = _search(_model("eos_min3"), c["x"], c["pos"], W, rl, return_trace=True)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, rl) >= d.B * c["S"]
    live = score > LIVE
    assert live[:, 0].all() and (seq[live][:, :d.L - 1] != 0).all()          # no live beam ends before step L-1


# ---- 4. bad endings
def test_bad_endings():
    name = cro.BAD_END_CASE
    c = cro.case(name)
    d, W = c["d"], c["W"]
    G = d.B * c["S"]
    rl = cro.rules(bad_end=cro.PINNED_BAD_END)
    m = _model(name)
    seq, lp, score, key, trace = _search(m, c["x"], c["pos"], W, rl, return_trace=True)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, rl) >= G
    live, tf = score > LIVE, _finish(seq)
    ended = (seq == 0).any(-1) & (tf < d.L - 1)
    bad = set(cro.PINNED_BAD_END)
    for g, k in np.argwhere(live & ended & (tf >= 1)):
        assert int(seq[g, k, tf[g, k] - 1]) not in bad, (g, k, seq[g, k])
    # the empty caption (word 0 at t = 0) is untouched by this rule: live, and its score is the plain search's
    pseq, plp, pscore = _plain(m, c["x"], c["pos"], W)
    empty, pempty = live & (seq[:, :, 0] == 0), (pscore > LIVE) & (pseq[:, :, 0] == 0)
    assert empty.any(1).all() and pempty.any(1).all()
    assert np.array_equal(score[empty], pscore[pempty])
    hit = sum(int(pseq[g, k, t - 1]) in bad for g, k in np.argwhere((pscore > LIVE) & (pseq == 0).any(-1)) for t in [_finish(pseq)[g, k]]
              if 1 <= t < d.L - 1)
    print("plain live beams that end on a listed word: %d" % hit)
    assert hit >= 1


# ---- 5. the length-scaled ranking
@pytest.mark.parametrize("form", list(cro.SCALE_FORMS))
def test_length_scale(form):
    name = cro.BAD_END_CASE
    c, o = cro.case(name), cro.scale_oracle64(form)
    d, W = c["d"], c["W"]
    G = d.B * c["S"]
    scale = cro.scale_table(d.L, form)
    rl = cro.rules(scale=scale)
    seq, lp, score, key, trace = _search(_model(name), c["x"], c["pos"], W, rl, return_trace=True)
    assert cro.check_admissible(trace, lp, score, key, seq, c["P"], c["xr"], d.L, W, rl) >= G
    live, tf = score > LIVE, _finish(seq)
    want = (score.astype(np.float32) * scale.astype(np.float32)[tf]).astype(np.float32)
    assert np.array_equal(key[live], want[live])                  # one fp32 multiply, bit for bit
    assert np.array_equal(key[~live], score[~live])
    assert (key[:, :-1] >= key[:, 1:]).all()
    assert (live[:, :-1] | ~live[:, 1:]).all() and live[:, 0].all()           # every live entry before every dead one
    # the order is the float64 oracle's where its margins pin it: the selection margin, and the gaps among its best W + 1 keys
    pinned = []
    for g in range(G):
        keys = -np.sort(-np.array([e["key"] for e in o["done"][g]], np.float64))[:W + 1]
        if o["margin"][g] >= MARGIN and np.min(keys[:-1] - keys[1:]) >= 2 * (d.L + 1) * LP_TOL:
            pinned.append(g)
    print("%s: %d of %d groups pinned, %d reordered against the score" % (form, len(pinned), G, cro.reordered_groups(dict(score=score))))
    assert pinned
    assert np.array_equal(seq[pinned], o["seq"][pinned])
    np.testing.assert_allclose(key[pinned], o["key"][pinned], atol=(d.L + 1) * LP_TOL)
    if cro.PINNED_REORDERED[form]:
        assert cro.reordered_groups(dict(score=score)) >= 1       # the ranking is not the one by score


# ---- 6. rules off: the searches without rules, bit for bit
@pytest.mark.parametrize("name", ["tiny_s3w3", "mid_s4w5"])
def test_rules_off_equal_the_searches_without_rules(name):
    c = cao.case(name)
    d, S, W = c["d"], c["S"], c["W"]
    m = make_model(d, c["P"], train=False)
    f, pos = _videos(c["x"]), torch.from_numpy(c["pos"]).cuda()
    wc = torch.from_numpy(np.ascontiguousarray(c["table"])).cuda()
    al = torch.from_numpy(np.asarray(c["masks"], np.int64)).cuda().reshape(d.B, S, -1)
    with torch.no_grad():
        want = m.beam_captions_allowed(*f, pos, wc, al, beam_size=W, return_trace=True)
        got = m.beam_captions_ruled(*f, pos, beam_size=W, word_cat=wc, allow=al, return_trace=True)
        same = m.beam_captions_ruled(*f, pos, beam_size=W, word_cat=wc, allow=al, no_repeat_ngram=d.L, return_trace=True)
        want_p = m.beam_captions_per_video(*f, pos, beam_size=W, return_trace=True)
        got_p = m.beam_captions_ruled(*f, pos, beam_size=W, return_trace=True)
        same_p = m.beam_captions_ruled(*f, pos, beam_size=W, no_repeat_ngram=d.L, return_trace=True)
    for w, g in ((want, got), (want_p, got_p), (want, same), (want_p, same_p)):
        # (an n-gram as long as the caption can never repeat: the selection under rules runs and bans nothing)
        for a, b in zip(w, (g[0], g[1], g[2], g[4])):
            assert torch.equal(a, b)
        assert torch.equal(g[3], g[2])                           # key == score


# ---- 7. the workspace and the trace
@pytest.mark.parametrize("name", ["tiny_n2", "mid_n3"])
def test_result_does_not_depend_on_the_workspace_or_the_trace(name):
    c = cro.case(name)
    m = make_model(c["d"], c["P"], train=False)
    rl = dict(c["rl"], min_length=2, bad_end=(3, 5), scale=cro.scale_table(c["d"].L, "avg1"))
    run = lambda **kw: _search(m, c["x"], c["pos"], c["W"], rl, **kw)      # noqa: E731
    first = run(return_trace=True)
    again = run(return_trace=True)
    (key, ws), = m._beam_rules_ws.items()
    m._beam_rules_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}   # NaNs and -1s, and larger
    dirty = run(return_trace=True)
    plain = run()
    for a, b_, c_ in zip(first, again, dirty):
        assert np.array_equal(a, b_) and np.array_equal(a, c_)
    assert len(plain) == 4 and all(np.array_equal(a, b_) for a, b_ in zip(first, plain))
    assert (first[2][:, 0] > LIVE).all()


# ---- 8. through the control chain
def test_beam_captions_ruled_with_templates_is_its_two_parts_done_by_hand():
    from controllable_xgating_amd import allow_masks, beam_captions_ruled_with_templates, length_scale_table, repeated_ngrams
    from tests import pos_control_oracle as pco
    from tests import pos_oracle as po
    from tests.pos_control_oracle import cuda_inputs, pos_model
    dp, dc = po.make_dims(**po.POS_CFG["tiny"]), pg.make_dims(**CFG["tiny"])
    assert (dp.B, dp.K, dp.R, dp.F1, dp.F2) == (dc.B, dc.K, dc.R, dc.F1, dc.F2)
    S, W = 3, 3
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    tm, _ = pco.seeded_templates(dp.B, S, dp.L, dp.C, seed=11)
    table = torch.from_numpy((np.arange(dc.V) % (dp.C - 1) + 1).astype(np.uint8))
    table[0] = 0
    wc = table.cuda()
    pm, cap = pos_model(dp, P, run), make_model(dc, pg.make_params(dc, logit_gain=32.0), train=False)
    fr, fo, fm = cuda_inputs(x)
    kw = dict(beam_size=W, no_repeat_ngram=1, min_length=1, bad_endings=[2, 3], length_scale=length_scale_table(dc.L, 1.0))
    for with_table in (False, True):
        got = beam_captions_ruled_with_templates(pm, cap, fr, fo, fm, tm, wc if with_table else None, **kw)
        assert len(got) == 5 and got[0].shape == (dp.B, S, W, dc.L) and got[3].shape == (dp.B, S, W) and got[4].shape == (dp.B, S)
        assert not any(t.requires_grad for t in got)
        with torch.no_grad():
            tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
            al = allow_masks(tm, dc.L).cuda() if with_table else None
            want = cap.beam_captions_ruled(fr, fo, fm, pos_feats.reshape(dp.B, S, -1), word_cat=wc if with_table else None, allow=al, **kw)
        assert torch.equal(got[4], tag_logp.sum(2))
        for a, b in zip(got[:4], want):                          # the same two calls: the same bits
            assert torch.equal(a, b)
        live = got[2] > LIVE
        assert not repeated_ngrams(got[0], 1)[live].any()
