"""The SCST rollout pair under train-mode dropout as ONE 2m-row pass (SAModel.sample_pair(..., {"one_pass": True}),
include/xgate_pair.h, docs/SCST_DROPOUT.md): rows [0, m) sample under the first seed of the model's counter, rows [m, 2m) decode
greedily under the second, each with the masks of an m-row call of its own.  Every case is checked against the oracle under the
two seeds (not against another HIP run), at the row counts where the split of the dropout descriptor meets another tiling, and
against the two-call path the option replaces.  p = 0.5 as in the reference's self-critical stage (starttrain.py:68,131)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import ws_state as wss
from tests.util import (CFG, ZERO_GRAD_PARAMS, assert_greedy_tokens_match, assert_sampled_tokens_match, check_sampled_rollout,
                        grad_misses, make_model, model_grads, oracle_rollouts, to_dev)

pytestmark = pytest.mark.gpu
P_DROP = 0.5
CALL = 100
ONE_PASS = {"one_pass": True, "return_greedy_logprobs": True}
EINVAL, EWORKSPACE = -1, -4                  # include/xgate.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def _case(cfg="mid", **over):
    """The greedy-friendly weights of tests/test_gpu_rollout_oracle.py (logit gain 8, no EOS bias: greedy rollouts run the full
    length over many distinct words with top-2 margins >= 1e-3 at p = 0.5 on `mid`); L = 12 on `mid`."""
    d = pg.make_dims(**dict(CFG[cfg], **dict({"L": 12} if cfg == "mid" else {}, **over)))
    Pn = pg.make_params(d, logit_gain=8.0)
    xn = pg.make_inputs(d, seed=0)
    u = pg.uniform("uni.ro", (d.L + 1, d.B), 41)
    reward = np.repeat(pg.uniform("rew.ro", (d.B, 1), 3, -1.0, 1.0), d.L, 1)
    return d, Pn, xn, u, reward


def _pair_seeds(d, Pn, call=CALL):
    """The two dropout seeds the pair takes, read from the product's own _run on a probe model in the same state."""
    probe = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    probe._call = call
    return probe._run(False).seed, probe._run(False).seed


def _pair(model, x, u, **opt):
    return model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                             dict({"uniforms": torch.from_numpy(u).cuda()}, **opt))


def _assert_logprobs_match(seq_h, lp_h, seq_o, logps_o, tol, what):
    """Per-step log-probs of a kernel's rollout vs the oracle's distributions `logps_o` (one (B,V) tensor per step): every step a
    row was alive at, up to and INCLUDING the row's first token difference from the oracle's rollout -- until then both stand in
    the same state, so the oracle's log-prob of the kernel's token is the reference.  Returns how many were compared."""
    seq_h, lp_h, seq_o = np.asarray(seq_h), np.asarray(lp_h), np.asarray(seq_o)
    n = 0
    for b in range(seq_h.shape[0]):
        for t in range(min(seq_h.shape[1], len(logps_o))):
            if t >= 1 and seq_h[b, t - 1] == 0:
                break
            ref = float(logps_o[t][b, int(seq_h[b, t])])
            assert abs(float(lp_h[b, t]) - ref) <= tol, (what, b, t, float(lp_h[b, t]), ref)
            n += 1
            if t >= seq_o.shape[1] or seq_h[b, t] != seq_o[b, t]:
                break
    return n


def _check_both_halves(out, d, Pn, xn, u, s1, s2, lp_tol=3e-4, draw_tol=3e-4, margin=1e-3):
    """Forward outputs of the one-pass pair against the oracle: the sampled half under s1, the greedy half under s2."""
    gen, slp, greedy, n, glp = out
    n_s, n_g = (int(v) for v in n.cpu())
    gen, slp, greedy, glp = (t.detach().cpu().numpy() for t in (gen, slp, greedy, glp))
    (s_o, lps), _ = oracle_rollouts(d, Pn, xn, u, s1, P_DROP)
    _, (g_o, lpg) = oracle_rollouts(d, Pn, xn, u, s2, P_DROP)
    assert_sampled_tokens_match(gen[:, :n_s], s_o, lps, u, tol=draw_tol)
    assert (g_o > 0).sum() > d.B
    assert_greedy_tokens_match(greedy[:, :n_g], g_o, lpg, margin=margin)
    assert not gen[:, n_s:].any() and not greedy[:, n_g:].any()
    assert _assert_logprobs_match(gen[:, :n_s], slp, s_o, lps, lp_tol, "sampled") >= d.B
    # the greedy rows' log-probs are what pins the masks of rows [m, 2m): a token may survive another mask, its log-prob does not
    assert _assert_logprobs_match(greedy[:, :n_g], glp, g_o, lpg, lp_tol, "greedy") > d.B
    return g_o


def test_one_pass_pair_vs_oracle_under_its_own_two_seeds():
    """Sampled half against the oracle under s1 with two BatchNorm updates (tokens, float64 replay log-probs within 3e-4, loss
    within 1e-4, every gradient, running statistics); greedy half against the oracle under s2 (tokens and per-step log-probs
    within 3e-4).  s1 != s2, and the oracle's greedy rollout under s1 is another one: shared masks would not pass."""
    from controllable_xgating_amd import RewardCriterion
    d, Pn, xn, u, reward = _case()
    x = to_dev(xn)
    s1, s2 = _pair_seeds(d, Pn)
    assert s1 != s2
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    model._call = CALL
    out = _pair(model, x, u, **ONE_PASS)
    gen, slp, greedy, n, glp = out
    n_s = int(n.cpu()[0])
    loss = RewardCriterion()(slp[:, :n_s], gen[:, :n_s], torch.from_numpy(reward[:, :n_s]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert model._call == CALL + 2
    check_sampled_rollout(model, d, Pn, xn, u, reward, gen[:, :n_s], slp[:, :n_s], loss.item(), s1, P_DROP, bn_updates=2)
    g_o = _check_both_halves(out, d, Pn, xn, u, s1, s2)
    _, (g_s1, _) = oracle_rollouts(d, Pn, xn, u, s1, P_DROP)
    assert not np.array_equal(g_s1, g_o)
    for bn in (model.two_spatial_encoder.visual_emb_rgb[1], model.two_spatial_encoder.visual_emb_opfl[1]):
        assert int(bn.num_batches_tracked) == 2


# m = 40: 80 rows, beyond 64 rows S2' moves into the step's first launch.  m = 68: 136 rows, beyond 128 rows the row-pass token
# choice, and the split falls inside the third 32-row tile (m = 12: inside the first).  odd: R = 20, the generic cell path with
# no packed kernel (pointwise gate and cell kernels).  bf16: the row pass on bf16 data.
@pytest.mark.parametrize("case", ["rows_80", "rows_136", "odd_generic_cells", "bf16_rows_24"])
def test_one_pass_pair_forward_vs_oracle_where_the_split_can_go_wrong(case):
    cfg, over = {"rows_80": ("mid", {"B": 40}), "rows_136": ("mid", {"B": 68}), "odd_generic_cells": ("odd", {}),
                 "bf16_rows_24": ("mid", {})}[case]
    bf16 = case == "bf16_rows_24"
    d, Pn, xn, u, _ = _case(cfg, **over)
    x = to_dev(xn)
    s1, s2 = _pair_seeds(d, Pn)
    assert s1 != s2
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP, precision="bf16" if bf16 else "fp32")
    model._call = CALL
    with torch.no_grad():
        out = _pair(model, x, u, **ONE_PASS)
    torch.cuda.synchronize()
    # bf16: log-probs within lp_tol = 1e-2 (test_tempered_sampling_vs_oracle).  Then an edge of the draw's CDF interval moves by at
    # most the sum of the probabilities' errors <= lp_tol, and two log-probs lp_tol off each may swap below a margin of 2 lp_tol.
    kw = dict(lp_tol=1e-2, draw_tol=1e-2, margin=2e-2) if bf16 else {}
    _check_both_halves(out, d, Pn, xn, u, s1, s2, **kw)


def test_one_pass_pair_equals_the_two_call_path():
    """Two models in the same _call state, one with the option: same n, same tokens in both halves; the sampled log-probs within
    3e-4 and every gradient within grad_misses' bounds (what test 1 holds each to against the oracle: the two forms run their
    products at other row counts); BatchNorm statistics equal after two updates each."""
    from controllable_xgating_amd import RewardCriterion
    d, Pn, xn, u, reward = _case()
    x = to_dev(xn)
    res = []
    for opt in (ONE_PASS, {"return_greedy_logprobs": True}):
        model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
        model._call = CALL
        gen, slp, greedy, n, glp = _pair(model, x, u, **opt)
        n_s = int(n.cpu()[0])
        loss = RewardCriterion()(slp[:, :n_s], gen[:, :n_s], torch.from_numpy(reward[:, :n_s]).cuda())
        loss.backward()
        torch.cuda.synchronize()
        assert model._call == CALL + 2
        res.append((model, gen, slp.detach(), greedy, n, glp, loss.item()))
    (ma, gen_a, slp_a, gr_a, n_a, glp_a, la), (mb, gen_b, slp_b, gr_b, n_b, glp_b, lb) = res
    assert torch.equal(n_a, n_b) and torch.equal(gen_a, gen_b) and torch.equal(gr_a, gr_b)
    n_s, n_g = (int(v) for v in n_a.cpu())
    np.testing.assert_allclose(slp_a.cpu().numpy(), slp_b.cpu().numpy(), atol=3e-4, rtol=0)
    np.testing.assert_allclose(glp_a.cpu().numpy()[:, :n_g], glp_b.cpu().numpy()[:, :n_g], atol=3e-4, rtol=0)
    assert abs(la - lb) < 1e-4, (la, lb)
    bad = grad_misses(model_grads(ma), model_grads(mb), skip=ZERO_GRAD_PARAMS)
    assert not bad, bad
    for mod in ("visual_emb_rgb", "visual_emb_opfl"):
        a, b = getattr(ma.two_spatial_encoder, mod)[1], getattr(mb.two_spatial_encoder, mod)[1]
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 2


def test_one_pass_pair_with_fixed_dropout_seed_gives_both_halves_that_seed():
    d, Pn, xn, u, _ = _case()
    x = to_dev(xn)
    s = 777001
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    model.dropout_seed = s
    with torch.no_grad():
        out = _pair(model, x, u, **ONE_PASS)
    torch.cuda.synchronize()
    _check_both_halves(out, d, Pn, xn, u, s, s)


@pytest.mark.parametrize("mode", ["train_p0", "eval_p05"])
def test_option_is_inert_without_dropout(mode):
    """At p = 0 in train mode and in eval mode at p = 0.5 the option takes today's paired pass: equal tensors."""
    d, Pn, xn, u, _ = _case()
    x = to_dev(xn)
    outs = []
    for opt in ({"return_greedy_logprobs": True}, ONE_PASS):
        model = make_model(d, P=Pn, train=mode == "train_p0", p_drop=0.0 if mode == "train_p0" else P_DROP)
        model._call = CALL
        with torch.no_grad():
            outs.append(_pair(model, x, u, **opt))
        torch.cuda.synchronize()
    assert len(outs[0]) == len(outs[1]) == 5
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert len(_pair(model, x, u, one_pass=True)) == 4


def test_one_pass_pair_does_not_depend_on_what_its_workspaces_held():
    """The call on the pool's fresh workspaces, then on the same buffers filled with NaN (tests/ws_state.py: everything but the
    synchronisation words; valid-but-wrong integers in the index ranges) with the same seeds: identical outputs."""
    d, Pn, xn, u, _ = _case()
    x = to_dev(xn)
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    runs = []
    for i in range(2):
        model._call = CALL
        with torch.no_grad():
            runs.append([t.clone() for t in _pair(model, x, u, **ONE_PASS)])
        torch.cuda.synchronize()
        assert wss.pool_sync_words_zero(model)
        if i == 0:
            assert wss.poison_pool(model) >= 2              # the m-row and the 2m-row workspace
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(runs[1][1]).all()) and bool(torch.isfinite(runs[1][4]).all())


def test_argument_checks_refuse_before_any_launch():
    """XG_EINVAL for d2->B != 2 d1->B, ws1 == ws2, null uniforms, temperature <= 0 and a null output, XG_EWORKSPACE for a short
    workspace -- on live device buffers, and the outputs keep their fill: nothing was enqueued."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pair as npr
    from controllable_xgating_amd.model import _stream, _ws_ptr
    d, Pn, xn, u, _ = _case()
    x = to_dev(xn)
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    B, T, dev = d.B, d.L + 1, x["feats_rgb"].device
    d1, d2, d3 = model._dims(B, d.K, T), model._dims(2 * B, d.K, T), model._dims(2 * B + 1, d.K, T)
    (wp1, wn1), (wp2, wn2) = _ws_ptr(model._pool.shared(d1, dev)), _ws_ptr(model._pool.shared(d2, dev))
    b1, keep = model._batch(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"])
    seq = torch.full((2 * B, T - 1), -7, dtype=torch.int64, device=dev)
    slp = torch.full((2 * B, T - 1), -7.0, device=dev)
    n = torch.full((2,), -7, dtype=torch.int32, device=dev)
    uni = torch.from_numpy(u).cuda().contiguous()
    ps, bn, run = model._params_struct(), model._bn_struct(), model._run(False)

    def call(da=d2, u_=nv.ptr(uni), temp=1.0, ws2=(wp2, wn2), ws1=(wp1, wn1), outs=None):
        o = [nv.ptr(seq), nv.ptr(slp), nv.ptr(n)] if outs is None else outs
        return npr.lib().xgpr_rollout_pair_videos(_stream(), C.byref(da), C.byref(ps), C.byref(bn), C.byref(b1), C.byref(run), 12345,
                                                  u_, temp, ws2[0], ws2[1], C.byref(d1), ws1[0], ws1[1], 0, o[0], o[1], o[2])

    assert call(da=d3, ws2=_ws_ptr(model._pool.shared(d3, dev))) == EINVAL and call(da=d1) == EINVAL      # (workspaces large enough)
    assert call(ws1=(wp2, wn2)) == EINVAL
    assert call(u_=None) == EINVAL
    assert call(temp=0.0) == EINVAL and call(temp=-1.0) == EINVAL
    for i in range(3):
        o = [nv.ptr(seq), nv.ptr(slp), nv.ptr(n)]
        o[i] = None
        assert call(outs=o) == EINVAL, i
    assert call(ws2=(wp2, 4096)) == EWORKSPACE and call(ws1=(wp1, 4096)) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((seq == -7).all()) and bool((slp == -7.0).all()) and bool((n == -7).all())
