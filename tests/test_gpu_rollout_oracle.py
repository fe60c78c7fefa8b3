"""Rollouts under train-mode dropout, tempered sampling and eval mode at drop_prob_lm = 0.5 -- each against the oracle, not
against another HIP run.  The reference runs SCST only at drop_prob_lm = 0.5 with both sample() calls in train mode
(starttrain.py:68,131, myutils.py:45-48), draws from the tempered distribution but gathers the UNTEMPERED log-prob
(SAModel.py:189-195), and evaluates a model built with drop_prob_lm = 0.5 switched to eval() (eval.py:57-73).  Gradients are
compared with the float64 oracle, exempting exactly what a flipped ReLU derivative feeds (tests/util.py: flip_exemptions)."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import (CFG, ZERO_GRAD_PARAMS, assert_greedy_tokens_match, assert_sampled_tokens_match, check_sampled_rollout,
                        grad_misses, make_model, model_grads, oracle_f64_with_flips, oracle_rollouts, to_dev)

pytestmark = pytest.mark.gpu
P_DROP = 0.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def _case(B=None, L=12, greedy=False):
    """`mid` (V = 500: not a multiple of the 32-column tile).  Sampling weights: an EOS bias so that sampled rows finish at
    different steps (greedy rollouts would all stop at t = 1).  greedy=True: logit gain 8, no EOS bias -- greedy rollouts run
    the full length over many distinct words with top-2 margins >= 1e-3 (measured at p = 0.5)."""
    d = pg.make_dims(**dict(CFG["mid"], L=L, **({} if B is None else {"B": B})))
    Pn = pg.make_params(d, logit_gain=8.0 if greedy else 1.0)
    Pn["logit.bias"] = Pn["logit.bias"].copy()
    Pn["logit.bias"][0] += 0.0 if greedy else 4.0
    xn = pg.make_inputs(d, seed=0)
    u = pg.uniform("uni.ro", (d.L + 1, d.B), 41)
    reward = np.repeat(pg.uniform("rew.ro", (d.B, 1), 3, -1.0, 1.0), d.L, 1)
    return d, Pn, xn, u, reward


def _sample(model, x, opt, reward):
    """model.sample in the model's mode; RewardCriterion backpropagated.  -> (seq, slp, loss)"""
    from controllable_xgating_amd import RewardCriterion
    seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], opt)
    n = seq.shape[1]
    loss = RewardCriterion()(slp, seq, torch.from_numpy(reward[:, :n]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return seq, slp, loss.item()


# ---------------------------------------------------------------- rollouts under train-mode dropout
def test_dropout_sampled_and_greedy_rollouts_vs_oracle():
    """model.sample in train mode at p = 0.5 with a fixed dropout seed: the sampled rollout against xo.sample(mode='sample',
    train=True, p=0.5, seed=s) and its float64 replay (log-probs, loss, every gradient, running statistics); the greedy
    rollout under another seed against xo.sample(mode='greedy', ..., seed=s') token for token.  The rollout form of the step
    applies dropout sites 5 / 6 / 7 in other epilogue instances than the teacher-forced form."""
    d, Pn, xn, u, reward = _case()
    x = to_dev(xn)
    s, s2 = 424242, 535353
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    model.dropout_seed = s
    seq, slp, loss = _sample(model, x, {"sample_max": 0, "uniforms": torch.from_numpy(u).cuda()}, reward)
    check_sampled_rollout(model, d, Pn, xn, u, reward, seq, slp, loss, s, P_DROP)
    d, Pn, xn, u, _ = _case(greedy=True)
    x = to_dev(xn)
    mg = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    mg.dropout_seed = s2
    with torch.no_grad():
        g_h, _ = mg.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    _, (g_o, lpg) = oracle_rollouts(d, Pn, xn, u, s2, P_DROP)
    assert (g_o > 0).sum() > d.B
    assert_greedy_tokens_match(g_h.cpu().numpy(), g_o, lpg)
    # the masks decide the tokens: the oracle's greedy rollout under the other seed, or without dropout, is another one
    _, (g_s, _) = oracle_rollouts(d, Pn, xn, u, s, P_DROP)
    _, (g_0, _) = oracle_rollouts(d, Pn, xn, u, s2, 0.0)
    assert not np.array_equal(g_s, g_o) and not np.array_equal(g_0, g_o)


def _pair_seeds(d, Pn, call):
    """The two dropout seeds sample_pair's two rollouts take, read from the product's own _run on a probe model in the same
    state (not from a copy of the formula)."""
    probe = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    probe._call = call
    return probe._run(False).seed, probe._run(False).seed


def test_sample_pair_with_dropout_vs_oracle_under_its_own_seeds():
    """sample_pair at p = 0.5 (the reference's SCST iteration, starttrain.py:131 + myutils.py:45): two rollouts with the two
    seeds of _call -- the sampled half against the oracle under the first (tokens, replay log-probs, loss, every gradient), the
    greedy half against the oracle under the second, and the running statistics equal two oracle BatchNorm updates."""
    d, Pn, xn, u, reward = _case(greedy=True)
    x = to_dev(xn)
    s1, s2 = _pair_seeds(d, Pn, 100)
    assert s1 != s2
    from controllable_xgating_amd import RewardCriterion
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    model._call = 100
    gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                            {"uniforms": torch.from_numpy(u).cuda()})
    n_s, n_g = (int(v) for v in n.cpu())
    loss = RewardCriterion()(slp[:, :n_s], gen[:, :n_s], torch.from_numpy(reward[:, :n_s]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    check_sampled_rollout(model, d, Pn, xn, u, reward, gen[:, :n_s], slp[:, :n_s], loss.item(), s1, P_DROP, bn_updates=2)
    _, (g_o, lpg) = oracle_rollouts(d, Pn, xn, u, s2, P_DROP)
    assert (g_o > 0).sum() > d.B
    assert_greedy_tokens_match(greedy[:, :n_g].cpu().numpy(), g_o, lpg)


def test_sample_pair_with_fixed_dropout_seed_gives_both_halves_that_seed():
    """With model.dropout_seed set, both rollouts of sample_pair at p > 0 take that one seed and so the same masks (a checker
    regenerates both from it); the two halves compare with the oracle under that seed."""
    d, Pn, xn, u, reward = _case(greedy=True)
    x = to_dev(xn)
    s = 777001
    model = make_model(d, P=Pn, train=True, p_drop=P_DROP)
    model.dropout_seed = s
    with torch.no_grad():
        gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                                {"uniforms": torch.from_numpy(u).cuda()})
    n_s, n_g = (int(v) for v in n.cpu())
    (s_o, lps), (g_o, lpg) = oracle_rollouts(d, Pn, xn, u, s, P_DROP)
    assert_sampled_tokens_match(gen[:, :n_s].cpu().numpy(), s_o, lps, u)
    assert (g_o > 0).sum() > d.B
    assert_greedy_tokens_match(greedy[:, :n_g].cpu().numpy(), g_o, lpg)


def test_scheduled_sampling_with_dropout_vs_oracle():
    """ss_prob = 0.5 at p = 0.5: the scheduled-sampling draws read the previous step's log-probs UNDER dropout
    (SAModel.py:89-99): same loss, log-probs and every gradient as xo.forward_xe(..., ss_prob=0.5, p=0.5, seed=s) in float64."""
    from controllable_xgating_amd import LanguageModelCriterion
    d = pg.make_dims(**CFG["mid"])
    T, s = d.L + 1, 246810
    u_sel, u_tok = pg.uniform("ss.sel", (T, d.B), 31), pg.uniform("ss.tok", (T, d.B), 32)
    Pn = pg.make_params(d)
    xn = pg.make_inputs(d, seed=0, ragged=True)

    def fn(P, xi, tr):
        its = []
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"],
                                     xi["seq_mask"], train=True, p=P_DROP, seed=s, running=xo.new_running(d), ss_prob=0.5,
                                     u_sel=u_sel, u_tok=u_tok, it_trace=its, relu_trace=tr)
        return xo.lm_criterion(logp, xi["seq"], xi["seq_mask"]), (logp.detach().numpy(), torch.stack(its).numpy())

    loss_o, (logp_o, its), g64, ex = oracle_f64_with_flips(Pn, xn, fn)
    assert (its != xn["seq"].T).sum() > 10                               # tokens really were replaced
    model = make_model(d, P=Pn, p_drop=P_DROP)
    model.dropout_seed = s
    model.ss_prob = 0.5
    model.ss_uniforms = (torch.from_numpy(u_sel).cuda(), torch.from_numpy(u_tok).cuda())
    x = to_dev(xn)
    logp, _ = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    loss = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_o) < 1e-4, (loss.item(), loss_o)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), logp_o, atol=3e-4)
    bad = grad_misses(model_grads(model), g64, skip=ZERO_GRAD_PARAMS, exempt=ex)
    assert not bad, bad


# ---------------------------------------------------------------- tempered sampling (temperature != 1)
# token-choice path per case (csrc/xg_model.hip: rollout loop):
#   fp32, 12 rows      -> the select prologue inside the step's first launch for steps 1 .. T-2, and the separate roll_select
#                         launch over the tile statistics for the last step (xgk_vocab_select_ok: <= 128 rows)
#   fp32, 136 rows     -> the row pass (more than 128 rows)
#   bf16, 12 rows      -> the row pass on bf16 data (gemm_mode != 0)
@pytest.mark.parametrize("temperature", [0.7, 1.3])
@pytest.mark.parametrize("path", ["in_step_and_roll_select", "row_pass_136_rows", "row_pass_bf16"])
def test_tempered_sampling_vs_oracle(path, temperature):
    """Tempered draw from supplied uniforms against xo.sample(mode='sample', temperature=T): tokens up to CDF-boundary draws;
    seqLogprobs equal the oracle's UNTEMPERED gather (SAModel.py:195) within 3e-4; the RewardCriterion backward equals an
    oracle replay of the same tokens (a tempered log-sum-exp kept for the backward would show in every logit gradient)."""
    bf16 = path == "row_pass_bf16"
    d, Pn, xn, u, reward = _case(B=136 if path == "row_pass_136_rows" else None)
    x = to_dev(xn)
    model = make_model(d, P=Pn, train=True, precision="bf16" if bf16 else "fp32")
    seq, slp, loss = _sample(model, x, {"sample_max": 0, "uniforms": torch.from_numpy(u).cuda(), "temperature": temperature},
                             reward)
    # bf16: the loss tolerance of configs[4] (1e-2) and the gradient bounds of its test (tests/test_gpu_fullsize.py: 5 % of the
    # scale, cosine 0.997)
    kw = dict(lp_tol=1e-2, loss_tol=1e-2, grad_kw=dict(rtol=5e-2, rtol_elem=5e-2, cos_min=0.997)) if bf16 else {}
    check_sampled_rollout(model, d, Pn, xn, u, reward, seq, slp, loss, 0, 0.0, temperature, **kw)
    if bf16:
        # ... and against the oracle that rounds where the kernels of this mode round (tests/bf16_oracle.py).  At `mid` only the
        # per-step products do (forward and data gradient; nothing reaches the 256 / 64 / 256 rule of the large products), the
        # float32 and the float64 emulation draw the same tokens at both temperatures and differ by 1e-5 in the log-probs and 1e-7
        # in the loss: the bounds are the fp32 path's own -- draws up to CDF-boundary ones against the EMULATED log-probs,
        # log-probs 3e-4, loss 1e-4, every gradient 2e-3 / 2e-6 and cosine 1 - 1e-5.
        from tests import bf16_oracle as bo
        tab = bo.policy_table(d, "rollout")
        sites = bo.rounding_sites(d, "rollout")
        assert len(sites) == 21 and all(tab[k][4] == "step" and k[1] in ("fwd", "dx") for k in sites), sites
        check_sampled_rollout(model, d, Pn, xn, u, reward, seq, slp, loss, 0, 0.0, temperature, policy=bo.hip_bf16_policy(d, "rollout"))


@pytest.mark.parametrize("temperature", [0.7, 1.3])
def test_tempered_sample_pair_vs_oracle(temperature):
    """sample_pair at p = 0 with a temperature: the paired 2m-row pass (split < rows: the sampled rows' logits in the alternative
    buffer).  Sampled half against the oracle's tempered draw and its replay, greedy half against the oracle's greedy rollout."""
    from controllable_xgating_amd import RewardCriterion
    d, Pn, xn, u, reward = _case(greedy=True)
    x = to_dev(xn)
    model = make_model(d, P=Pn, train=True)
    gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                            {"uniforms": torch.from_numpy(u).cuda(), "temperature": temperature})
    n_s, n_g = (int(v) for v in n.cpu())
    loss = RewardCriterion()(slp[:, :n_s], gen[:, :n_s], torch.from_numpy(reward[:, :n_s]).cuda())
    loss.backward()
    torch.cuda.synchronize()
    check_sampled_rollout(model, d, Pn, xn, u, reward, gen[:, :n_s], slp[:, :n_s], loss.item(), 0, 0.0, temperature,
                          bn_updates=2)
    _, (g_o, lpg) = oracle_rollouts(d, Pn, xn, u, 0, 0.0)
    assert (g_o > 0).sum() > d.B
    assert_greedy_tokens_match(greedy[:, :n_g].cpu().numpy(), g_o, lpg)


# ---------------------------------------------------------------- eval mode of a model built with drop_prob_lm = 0.5
def test_eval_mode_dropout_half_xe_vs_oracle():
    """drop_prob_lm = 0.5 switched to eval() (eval.py:57-73): XgRun carries train = 0, drop_p = 0.5 and no site may drop --
    encoder sites 0-4 and classifier site 8 included.  Log-probs, category log-probs and losses equal the oracle's eval-mode
    forward (no masks) on non-trivial running statistics."""
    from controllable_xgating_amd import ClassiferCriterion, LanguageModelCriterion
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d)
    xn = pg.make_inputs(d, seed=0, ragged=True)
    running = xo.new_running(d)
    model = make_model(d, P=Pn, p_drop=P_DROP, train=False)
    for mod in ("rgb", "opfl"):
        pre = xo.ENC + f"visual_emb_{mod}.1."
        running[pre + "running_mean"] = torch.from_numpy(pg.uniform(f"rm.{mod}", (d.R,), 9, -0.3, 0.3))
        running[pre + "running_var"] = torch.from_numpy(pg.uniform(f"rv.{mod}", (d.R,), 9, 0.5, 2.0))
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        bn.running_mean.copy_(running[pre + "running_mean"])
        bn.running_var.copy_(running[pre + "running_var"])
    xi = xo.to_torch_inputs(xn)
    with torch.no_grad():
        lo, co, _ = xo.forward_xe(xo.to_torch_params(Pn), xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"],
                                  xi["seq"], xi["seq_mask"], train=False, p=P_DROP, seed=0, running=running)
        l_xe_o = xo.lm_criterion(lo, xi["seq"], xi["seq_mask"]).item()
        l_cls_o = xo.cls_criterion(co, xi["cap_classes"], xi["seq_mask"], xi["class_mask"]).item()
    x = to_dev(xn)
    with torch.no_grad():
        logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
        l_xe = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"]).item()
        l_cls = ClassiferCriterion()(cat, x["cap_classes"], x["seq_mask"], x["class_mask"]).item()
    assert abs(l_xe - l_xe_o) < 1e-4 and abs(l_cls - l_cls_o) < 1e-4, (l_xe, l_xe_o, l_cls, l_cls_o)
    np.testing.assert_allclose(logp.cpu().numpy(), lo.numpy(), atol=3e-4, rtol=0)
    np.testing.assert_allclose(cat.cpu().numpy(), co.numpy(), atol=1e-4, rtol=0)
