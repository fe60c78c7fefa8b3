"""The captioner's beam search whose words must follow a POS template on the MI355X: SAModel.beam_captions_allowed
(include/xgate_beam_allow.h) judged by tests/cap_allow_oracle.py -- the search of include/xgate_beam_control.h on the repeated batch
with step 2 replaced: the softmax over the allowed words, 1000 off every other word.  First the kernel's OWN trace replayed in
float64 on every group (check_admissible: none excused), then what the header promises, exactly: every token of a live beam allowed
at its position, the forced length, a log-probability of exactly 0 at a single-word step, the W distinct words of a row with fewer
than W allowed ones, the tie rule under a mask (the threshold selection's overflow fallback included), the empty set and the zero
mask as 0xFFFFFFFF, all-ones masks against beam_captions_per_video, the float64 search where its margin pins the tokens, workspace
and trace independence, and control.beam_captions_following_templates against its two parts done by hand.

Bounds: log-probabilities 3e-4 (the project's bound for this model), a sum of k of them k * 3e-4.  Cases, tables, templates and the
pinned counts (chosen and counted on the CPU): tests/cap_allow_oracle.py and tests/test_cap_allow_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_allow_oracle as cao
from tests import cap_beam_oracle as cbo
from tests.util import CFG, make_model

pytestmark = pytest.mark.gpu
LP_TOL, LIVE, MARGIN, ANY = cao.LP_TOL, cao.LIVE, cao.MARGIN, cao.ANY
TW_CAND = 32                                                     # the threshold selection's candidate list


def _videos(x):
    return tuple(torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))


def _dev(table, masks, B, S):
    return torch.from_numpy(np.ascontiguousarray(table)).cuda(), torch.from_numpy(np.asarray(masks, np.int64)).cuda().reshape(B, S, -1)


def _search(m, x, pos, table, masks, W, **kw):
    """beam_captions_allowed, as numpy viewed over the G = B S groups: [seq (G,W,L), seq_logp, score (G,W)[, trace (G,L,W,2)]]."""
    B, S = pos.shape[:2]
    wc, al = _dev(table, masks, B, S)
    with torch.no_grad():
        out = m.beam_captions_allowed(*_videos(x), torch.from_numpy(pos).cuda(), wc, al, beam_size=W, **kw)
    torch.cuda.synchronize()
    assert out[0].shape[:3] == (B, S, W) and out[2].shape == (B, S, W)
    return [v.cpu().numpy().reshape((B * S,) + tuple(v.shape[2:])) for v in out]


@functools.lru_cache(maxsize=None)
def _result(name):
    """A case's search on the device with its trace, run once and shared (nobody writes into it): (seq, lp, score, trace)."""
    c = cao.case(name)
    return tuple(_search(make_model(c["d"], c["P"], train=False), c["x"], c["pos"], c["table"], c["masks"], c["W"], return_trace=True))


# ---- 1. the kernel's own trace, judged in float64 on every group; adherence, exactly
@pytest.mark.parametrize("name", list(cao.CASES))
def test_own_trace_is_admissible_and_live_beams_adhere(name):
    from controllable_xgating_amd import template_adherence
    c = cao.case(name)
    d, S, W = c["d"], c["S"], c["W"]
    G = d.B * S
    seq, lp, score, trace = _result(name)
    assert seq.shape == (G, W, d.L) and seq.dtype == np.int64 and lp.shape == seq.shape and score.shape == (G, W)
    assert trace.shape == (G, d.L, W, 2) and trace.dtype == np.int32
    assert seq.min() >= 0 and seq.max() < d.V and (score[:, :-1] >= score[:, 1:]).all() and np.isfinite(score).all() and np.isfinite(lp).all()
    checked = cao.check_admissible(trace, lp, score, seq, c["P"], c["xr"], d.L, W, c["table"], c["masks"])
    assert checked >= G
    # every token of every live beam is allowed at its position: exact, no row excused -- by the package's own check on the device
    # and by the oracle's predicate on the host
    live = score > LIVE
    assert live[:, 0].all()                                      # every group has a live beam
    wc, al = _dev(c["table"], c["masks"], d.B, S)
    adh = template_adherence(torch.from_numpy(seq).cuda().reshape(d.B, S, W, d.L), al, wc).cpu().numpy().reshape(G, W)
    assert adh[live].all(), np.argwhere(live & ~adh)
    ok = cao.allowed_words(c["table"], c["masks"])
    for g, k in np.argwhere(live):
        for t, w in enumerate(seq[g, k]):
            assert ok[g, t, w], (g, k, t, w)
            if w == 0:
                break
    for g in range(G):                                           # a group's live beams are distinct captions
        rows = [tuple(r) for r, s in zip(seq[g], score[g]) if s > LIVE]
        assert len(set(rows)) == len(rows), g


# ---- 2. the forced length and the single-word step
@pytest.mark.parametrize("name", ["tiny_s3w3", "mid_s4w5"])
def test_plain_templates_force_length_and_tags(name):
    c = cao.case(name)
    d = c["d"]
    seq, lp, score, _ = _result(name)
    single = int(np.flatnonzero(c["table"] == cao.SINGLE)[0])
    forced = zeros = 0
    for g, kind in enumerate(c["kinds"]):
        for k in np.flatnonzero(score[g] > LIVE):
            s, n = seq[g, k], c["n"][g]
            if kind == "plain":                                  # n < L single tags, then tag 0: exactly n words, the finish at step n
                assert n < d.L and (s[:n] != 0).all() and (s[n:] == 0).all() and (lp[g, k, n + 1:] == 0).all(), (g, k, s, n)
                assert c["table"][s[:n]].tolist() == c["tags"][g, :n].tolist(), (g, k)
                assert lp[g, k, n] == 0.0                        # word 0 is the only word of category 0
                forced += 1
            for t in range(d.L):                                 # a step whose allowed set is one word: lp == 0.0f exactly
                if c["masks"][g, t] == 1 << cao.SINGLE and (s[:t] != 0).all():
                    assert s[t] == single and lp[g, k, t] == 0.0, (g, k, t, lp[g, k, t])
                    zeros += 1
    assert forced and zeros


# ---- 3. a row with fewer allowed words than W
def test_two_word_category_at_three_beams():
    """Position 0 admits the two words of PAIR in every group: the one row of step 0 yields them and, third, a word with the -1000;
    the whole trace is the float64 oracle's wherever its margin pins it."""
    c = cao.short_row_case()
    d, S, W, o = c["d"], c["S"], c["W"], c["oracle"]
    G = d.B * S
    assert W == 3
    seq, lp, score, trace = _search(make_model(d, c["P"], train=False), c["x"], c["pos"], c["table"], c["masks"], W, return_trace=True)
    pair = set(np.flatnonzero(c["table"] == cao.PAIR).tolist())
    for g in range(G):
        assert set(trace[g, 0, :2, 0].tolist()) == pair and trace[g, 0, 2, 0] not in pair and trace[g, 0, 2, 0] != 1, g
    # the third candidate's r carries the -1000: every beam that starts with it is dead, and its first r lies below LIVE
    third = seq[:, :, 0] == trace[:, 0, 2:3, 0]
    assert (score[third] < LIVE).all() and (lp[:, :, 0][third] < LIVE).all() and (lp[:, :, 0][~third] > LIVE).all()
    assert cao.check_admissible(trace, lp, score, seq, c["P"], c["xr"], d.L, W, c["table"], c["masks"]) >= G
    ok = np.flatnonzero(o["margin"] >= MARGIN)
    assert 5 * len(ok) >= 4 * G                                  # a condition on the inputs (tests/test_cap_allow_cpu.py), no measurement
    assert np.array_equal(trace[ok], o["trace"][ok]) and np.array_equal(seq[ok], o["seq"][ok])
    np.testing.assert_allclose(lp[ok], o["seq_logp"][ok], atol=LP_TOL)


# ---- 4. the tie rule under a mask
def _flat_head(P):
    P = dict(P)
    P["logit.weight"] = np.zeros_like(P["logit.weight"])
    P["logit.bias"] = np.full_like(P["logit.bias"], 0.25)
    return P


@pytest.mark.parametrize("V", [61, 20001])
def test_all_equal_logits_follow_the_tie_rule_among_allowed_words(V):
    """Every logit equal, half the vocabulary allowed: the allowed words tie at the threshold -- at V = 61 inside the candidate
    list, at V = 20001 more of them than it holds: the whole workgroup takes the insertion path -- and the lowest allowed indices
    win; lp = -log(number allowed)."""
    d = pg.make_dims(**dict(CFG["tiny"], B=2, V=V))
    S, W = 2, 3
    P, x, pos = _flat_head(pg.make_params(d)), pg.make_inputs(d, seed=3), cao.make_pos(d, S, 5)
    table = np.where(np.arange(V) % 2 == 1, 6, 5).astype(np.uint8)          # odd words: category 6
    table[0], table[1] = 0, 1
    masks = np.full((d.B * S, d.L), 1 << 6, np.int64)
    masks[1] = (1 << 5) | 1                                                 # group 1: the even words, word 0 among them
    n_odd = int(((np.arange(V) % 2 == 1) & (np.arange(V) > 1)).sum())
    n_even = V - 1 - n_odd
    assert W < n_odd <= TW_CAND and W < n_even <= TW_CAND if V == 61 else n_odd > TW_CAND and n_even > TW_CAND
    seq, lp, score, trace = _search(make_model(d, P, train=False), x, pos, table, masks, W, return_trace=True)
    o = cao.allowed_beam_captions(P, cao.repeated(x, pos), d.L, S, W, table, masks)
    assert np.array_equal(trace, o["trace"]) and np.array_equal(seq, o["seq"])
    np.testing.assert_allclose(lp, o["seq_logp"], atol=1e-5)
    assert (trace[0, 0, :, 0] == [3, 5, 7]).all() and (trace[1, 0, :, 0] == [0, 2, 4]).all()
    np.testing.assert_allclose(lp[0, 0, 0], -np.log(n_odd), atol=1e-5)
    np.testing.assert_allclose(score[1, 0], -np.log(n_even), atol=1e-5)      # group 1's best beam: word 0 at once


# ---- 5. the empty category and the zero mask are 0xFFFFFFFF
@pytest.mark.parametrize("name", ["tiny_s3w3", "v20001", "v38500"])
def test_empty_category_and_zero_mask_equal_all_ones(name):
    c = cao.case(name)
    d = c["d"]
    m = c["masks"].copy()
    fallback = (m == 0) | (m == 1 << cao.EMPTY)
    assert fallback.any() and (m == 0).any() and (m == 1 << cao.EMPTY).any()
    m[fallback] = ANY
    want = _search(make_model(d, c["P"], train=False), c["x"], c["pos"], c["table"], m, c["W"], return_trace=True)
    for a, b in zip(_result(name), want):
        assert np.array_equal(a, b)


# ---- 6. all-ones masks: the unconstrained search
@pytest.mark.parametrize("name", cao.PINNED)
def test_all_ones_masks_against_beam_captions_per_video(name):
    c = cao.case(name)
    d, S, W = c["d"], c["S"], c["W"]
    G = d.B * S
    m = make_model(d, c["P"], train=False)
    seq, lp, score, trace = _search(m, c["x"], c["pos"], c["table"], np.full((G, d.L), ANY, np.int64), W, return_trace=True)
    with torch.no_grad():
        want = m.beam_captions_per_video(*_videos(c["x"]), torch.from_numpy(c["pos"]).cuda(), beam_size=W, return_trace=True)
    seq_r, lp_r, score_r, trace_r = (v.cpu().numpy().reshape((G,) + tuple(v.shape[2:])) for v in want)
    assert np.array_equal(seq, seq_r)                                        # on every group
    margin = cbo.beam_captions(c["P"], c["xr"], d.L, W, dtype=torch.float64)["margin"]
    ok = np.flatnonzero(margin >= MARGIN)
    assert 5 * len(ok) >= 4 * G
    assert np.array_equal(trace[ok], trace_r[ok])
    np.testing.assert_allclose(lp, lp_r, atol=LP_TOL)
    np.testing.assert_allclose(score, score_r, atol=(d.L + 1) * LP_TOL)


# ---- 7. the float64 constrained search where its margin pins the tokens
@pytest.mark.parametrize("name", cao.PINNED)
def test_pinned_groups_against_the_float64_search(name):
    c, o = cao.case(name), cao.case_oracle(name)
    seq, lp, score, _ = _result(name)
    ok = np.flatnonzero(o["margin"] >= MARGIN)
    print("%d of %d groups pinned" % (len(ok), len(o["margin"])))
    assert 5 * len(ok) >= 4 * len(o["margin"])                               # a condition on the inputs, not a measurement
    assert np.array_equal(seq[ok], o["seq"][ok]), np.flatnonzero((seq[ok] != o["seq"][ok]).any((1, 2)))
    np.testing.assert_allclose(lp[ok], o["seq_logp"][ok], atol=LP_TOL)
    np.testing.assert_allclose(score[ok], o["score"][ok], atol=(c["d"].L + 1) * LP_TOL)


# ---- 8. the workspace and the trace
@pytest.mark.parametrize("name", ["tiny_s3w3", "mid_s4w5"])
def test_result_does_not_depend_on_the_workspace_or_the_trace(name):
    c = cao.case(name)
    m = make_model(c["d"], c["P"], train=False)
    run = lambda **kw: _search(m, c["x"], c["pos"], c["table"], c["masks"], c["W"], **kw)      # noqa: E731
    first = run(return_trace=True)
    again = run(return_trace=True)
    (key, ws), = m._beam_allow_ws.items()
    m._beam_allow_ws = {key: torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=ws.device)}   # NaNs and -1s, and larger
    dirty = run(return_trace=True)
    plain = run()
    for a, b_, c_, e in zip(first, again, dirty, _result(name)):
        assert np.array_equal(a, b_) and np.array_equal(a, c_) and np.array_equal(a, e)
    assert len(plain) == 3 and all(np.array_equal(a, b_) for a, b_ in zip(first, plain))


# ---- 9. through the control chain
def test_beam_captions_following_templates_is_its_two_parts_done_by_hand():
    from controllable_xgating_amd import allow_masks, beam_captions_following_templates, template_adherence
    from tests import pos_control_oracle as pco
    from tests import pos_oracle as po
    from tests.pos_control_oracle import cuda_inputs, pos_model
    dp, dc = po.make_dims(**po.POS_CFG["tiny"]), pg.make_dims(**CFG["tiny"])
    assert (dp.B, dp.K, dp.R, dp.F1, dp.F2) == (dc.B, dc.K, dc.R, dc.F1, dc.F2)
    S, W = 3, 3
    P, run, x = po.make_params(dp), po.make_running(dp), po.make_inputs(dp, seed=20, ragged=True)
    tm, _ = pco.seeded_templates(dp.B, S, dp.L, dp.C, seed=11)
    table = torch.from_numpy((np.arange(dc.V) % (dp.C - 1) + 1).astype(np.uint8))       # every tag but 0 has words; word 0 alone ends
    table[0] = 0
    wc = table.cuda()
    pm, cap = pos_model(dp, P, run), make_model(dc, pg.make_params(dc, logit_gain=32.0), train=False)
    fr, fo, fm = cuda_inputs(x)
    seq, lp, score, tscore = beam_captions_following_templates(pm, cap, fr, fo, fm, tm, wc, beam_size=W)
    assert seq.shape == (dp.B, S, W, dc.L) and lp.shape == seq.shape and score.shape == (dp.B, S, W) and tscore.shape == (dp.B, S)
    assert not any(t.requires_grad for t in (seq, lp, score, tscore))
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pm.sample_forced(fr, fo, fm, tm, collect_states=False, trim=False)
        al = allow_masks(tm, dc.L).cuda()
        want = cap.beam_captions_allowed(fr, fo, fm, pos_feats.reshape(dp.B, S, -1), wc, al, beam_size=W)
    assert torch.equal(tscore, tag_logp.sum(2))
    for a, b in zip((seq, lp, score), want):                                 # the same two calls: the same bits
        assert torch.equal(a, b)
    live = score > LIVE
    assert live[:, :, 0].all() and template_adherence(seq, al, wc)[live].all()
    # the captions carry their templates' tags: word by word up to the template's end
    tags = wc.long()[seq]                                                    # (B,S,W,L)
    tmd = torch.as_tensor(tm).cuda().long()
    tmd = torch.nn.functional.pad(tmd, (0, dc.L - tmd.shape[2])).unsqueeze(2).expand_as(tags)
    upto = torch.cat([torch.ones_like(tmd[..., :1], dtype=torch.bool), (tmd != 0).long().cumprod(3).bool()[..., :-1]], 3)
    assert ((tags == tmd) | ~upto)[live].all()
