"""Self-critical training on S rollouts per video on the MI355X: SAModel.rollout_per_video and PerVideoRewardCriterion (include/
xgate_scst_video.h) against the composed oracle of tests/cap_scst_video_oracle.py -- the tokens against the oracle's own draw from the
same uniforms, then the float64 oracle replaying the kernel's tokens: seqLogprobs, the loss, every parameter gradient and the BatchNorm
running statistics --, under dropout, in eval mode, at a temperature, against sample_per_video and against sample() + RewardCriterion,
on a workspace full of NaNs, and through Trainer.train_batch.

Bounds (tests.util.check_sampled_rollout): tokens under assert_sampled_tokens_match (3e-4 of a CDF edge), at most 2 rows of a case
excused -- tools/cap_scst_video_draw_check.py: the float32 and the float64 composed oracle draw the same tokens in every row of every
multi-row case at p 0 and 0.5 and temperature 1.0 and 0.7 --; seqLogprobs 3e-4, the loss 1e-4, gradients by grad_misses at its
defaults (rtol 2e-3, atol 2e-6, cosine >= 1 - 1e-5) under the ReLU-flip exemptions, running statistics 1e-5 against ONE update from the
B videos.  The cases and what each reaches: tests/cap_scst_video_oracle.py, checked without a GPU in tests/test_cap_scst_video_cpu.py."""
import argparse
import functools

import numpy as np
import pytest
import torch

from oracle import xgate_oracle as xo
from tests import cap_scst_video_oracle as svo
from tests.util import (ZERO_GRAD_PARAMS, assert_grads_close, assert_sampled_tokens_match, grad_misses, make_model, model_grads,
                        oracle_f64_with_flips)

pytestmark = pytest.mark.gpu

MAX_EXCUSED_ROWS = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The device inputs of a case: (feats_rgb, feats_opfl, feat_mask, pos_feats (B,S,R), uniforms (L + 1, M)); made once, shared."""
    d, S, _, xv, pos, u = svo.case_inputs(name)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    return t(xv["feats_rgb"]), t(xv["feats_opfl"]), t(xv["feat_mask"]), t(pos).reshape(d.B, S, d.R), t(u)


@functools.lru_cache(maxsize=None)
def _scores(name):
    """One score per row (B,S) and a base per video (B,), fixed."""
    d, S = svo.dims(name)
    rng = np.random.default_rng(5)
    return rng.random((d.B, S)).astype(np.float32), rng.random(d.B).astype(np.float32)


def _model(name, p=0.0, seed=None, train=True):
    d, _, P = svo.case_inputs(name)[:3]
    m = make_model(d, P, p_drop=p, train=train)
    if seed is not None:
        m.dropout_seed = seed
    return m


def _baseline_args(name, baseline):
    """(the criterion's `baseline` argument, the numpy rule, its base) for "mean_others", None or "given"."""
    score, base = _scores(name)
    if baseline == "given":
        return torch.from_numpy(base).cuda(), "given", base
    return baseline, baseline, None


def _iteration(model, name, baseline="mean_others", temperature=1.0, crit=None):
    """rollout + criterion + backward; returns (seq (M,n), slp (M,n), loss, advantages (B,S), n), numpy."""
    from controllable_xgating_amd import PerVideoRewardCriterion
    a = _dev(name)
    model.zero_grad(set_to_none=True)
    seq, slp, n = model.rollout_per_video(*a[:4], temperature=temperature, uniforms=a[4])
    crit = crit or PerVideoRewardCriterion()
    loss = crit(slp, seq, torch.from_numpy(_scores(name)[0]).cuda(), n=n, baseline=_baseline_args(name, baseline)[0])
    loss.backward()
    torch.cuda.synchronize()
    k = int(n.item())
    M = seq.shape[0] * seq.shape[1]
    assert seq.dtype == torch.int64 and tuple(slp.shape) == tuple(seq.shape) and bool((seq[:, :, k:] == 0).all())
    return (seq.reshape(M, -1)[:, :k].cpu().numpy(), slp.detach().reshape(M, -1)[:, :k].cpu().numpy(), float(loss.item()),
            crit.last_advantage.cpu().numpy(), k)


def _check_against_oracle(model, name, out, baseline="mean_others", temperature=1.0, train=True, p=0.0, seed=0, grad_kw=None):
    """tests.util.check_sampled_rollout for the composed oracle."""
    d, S, Pn, xv, pos, u = svo.case_inputs(name)
    seq, slp, loss, adv, k = out
    M = d.B * S
    s_o, lps = svo.case_draw(name, train, p, seed, temperature)
    rows = assert_sampled_tokens_match(seq, s_o, lps, u, temperature)
    print("%s: width %d (oracle %d), rows excused %s" % (name, k, s_o.shape[1], rows))
    assert len(rows) <= MAX_EXCUSED_ROWS, rows
    _, rule, base = _baseline_args(name, baseline)
    adv_o = svo.advantages(_scores(name)[0], rule, base)
    np.testing.assert_allclose(adv, adv_o, atol=1e-6)
    forced = torch.from_numpy(seq)

    def fn(P, xi, tr):
        running = xo.new_running(d)
        so, lp = svo.composed_sample(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], S, d.L, "replay",
                                     forced=forced, train=train, p=p, seed=seed, running=running, relu_trace=tr)
        reward = torch.from_numpy(np.repeat(adv_o.reshape(M, 1), k, 1)).to(lp.dtype)
        return xo.reward_criterion(lp, so, reward), (lp.detach().numpy(), running)

    loss_o, (lp_o, running), g64, ex = oracle_f64_with_flips(Pn, svo.oracle_inputs(name), fn)
    m = svo.reward_mask(seq)
    print("%s: loss %.6f (oracle %.6f), worst log-prob %.2e" % (name, loss, loss_o, np.abs(slp[m] - lp_o[m]).max()))
    np.testing.assert_allclose(slp[m], lp_o[m], atol=3e-4)
    assert abs(loss - loss_o) < 1e-4, (loss, loss_o)
    report = {}
    bad = grad_misses(model_grads(model), g64, skip=ZERO_GRAD_PARAMS, exempt=ex, report=report, **(grad_kw or {}))
    print("%s: worst gradient %s" % (name, max(report.items(), key=lambda kv: kv[1][2]) if report else None))
    assert not bad, bad
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), running[pre + "running_mean"].numpy(), atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), running[pre + "running_var"].numpy(), atol=1e-5)
        assert int(bn.num_batches_tracked) == (1 if train else 0)


@pytest.mark.parametrize("name", list(svo.CASES))
def test_rollout_criterion_gradients_and_running_statistics_vs_composed_oracle(name):
    """Train mode, p = 0 (mid_s1: S = 1, where "mean_others" does not exist: a given base per video)."""
    baseline = "given" if svo.CASES[name][2] == 1 else "mean_others"
    model = _model(name)
    out = _iteration(model, name, baseline)
    _check_against_oracle(model, name, out, baseline)


def test_dropout_masks_match_the_composed_oracle():
    """p = 0.5, seed pinned: the encoder's sites draw by element index in the B-video tensors, the decoder's by row in the M-row
    tensors -- the composed oracle under ONE seed.  Another seed draws other tokens or other log-probabilities."""
    name, seed = "mid_b3_s5", 123457
    model = _model(name, p=0.5, seed=seed)
    out = _iteration(model, name)
    _check_against_oracle(model, name, out, p=0.5, seed=seed)
    other = _model(name, p=0.5, seed=seed + 1)
    a = _dev(name)
    with torch.no_grad():
        seq2, slp2, n2 = other.rollout_per_video(*a[:4], uniforms=a[4], trim=True)
    k = min(out[0].shape[1], seq2.shape[2])
    s2, l2 = seq2.reshape(-1, seq2.shape[2])[:, :k].cpu().numpy(), slp2.reshape(-1, slp2.shape[2])[:, :k].cpu().numpy()
    assert (s2 != out[0][:, :k]).any() or np.abs(l2 - out[1][:, :k]).max() > 1e-3


@pytest.mark.parametrize("name", ["tiny_s5", "mid_b3_s5"])
def test_eval_mode_vs_composed_oracle(name):
    """Eval mode: BatchNorm reads the running statistics and leaves them alone; the backward works as in train mode."""
    model = _model(name, train=False)
    out = _iteration(model, name)
    _check_against_oracle(model, name, out, train=False)
    bn = model.two_spatial_encoder.visual_emb_rgb[1]
    assert int(bn.num_batches_tracked) == 0 and float(bn.running_mean.abs().max()) == 0.0


@pytest.mark.parametrize("name", ["mid_b3_s5", "tiny_s5"])
def test_temperature(name):
    """Tokens drawn from softmax(logits / 0.7), the untempered log-probability gathered."""
    model = _model(name)
    out = _iteration(model, name, temperature=0.7)
    _check_against_oracle(model, name, out, temperature=0.7)
    plain = _iteration(_model(name), name)
    assert plain[0].shape != out[0].shape or (plain[0] != out[0]).any()


# ---- the criterion
def _criterion_inputs(B, S, L, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    slp = -torch.rand(B, S, L, generator=g) * 5
    seq = torch.randint(0, 6, (B, S, L), generator=g)
    seq[0, 0] = 0                                            # a row that ends at its first word
    dead = torch.cumsum((seq == 0).long(), 2) > 0            # a rollout's rows: zeros behind the first end
    seq[dead] = 0
    score, base = torch.rand(B, S, generator=g), torch.rand(B, generator=g)
    nd = None if n is None else torch.tensor([n], dtype=torch.int32).cuda()
    return slp.cuda().requires_grad_(True), seq.cuda(), score.cuda(), base.cuda(), nd


# (3, 5, 7): one wave's worth; (70, 2, 4): more videos than the final pass has lanes; (2, 40, 7): S L = 280 > 256 threads, S > 32;
# (1, 1, 1) and n below L
_CRIT_SHAPES = [(3, 5, 7, None), (70, 2, 4, 3), (2, 40, 7, 5), (1, 1, 1, None), (5, 300, 3, 2)]


@pytest.mark.parametrize("B,S,L,n,baseline", [sh + (b,) for sh in _CRIT_SHAPES for b in ("mean_others", None, "given")
                                              if not (b == "mean_others" and sh[1] < 2)])
def test_criterion_vs_numpy(B, S, L, n, baseline):
    from controllable_xgating_amd import PerVideoRewardCriterion
    slp, seq, score, base, nd = _criterion_inputs(B, S, L, n)
    crit = PerVideoRewardCriterion()
    loss = crit(slp, seq, score, n=nd, baseline=base if baseline == "given" else baseline)
    (3.0 * loss).backward()
    adv_o = svo.advantages(score.cpu().numpy(), baseline, base.cpu().numpy())
    loss_o, dslp_o = svo.criterion(slp.detach().cpu().numpy(), seq.cpu().numpy(), adv_o, n)
    np.testing.assert_allclose(crit.last_advantage.cpu().numpy(), adv_o, atol=1e-6)
    assert abs(loss.item() - loss_o) <= 1e-5 * max(1.0, abs(loss_o)), (loss.item(), loss_o)
    np.testing.assert_allclose(slp.grad.cpu().numpy(), 3.0 * dslp_o, rtol=1e-5, atol=1e-7)


def test_criterion_twice_is_bit_identical_and_needs_no_zeroed_output():
    from controllable_xgating_amd import PerVideoRewardCriterion
    slp, seq, score, base, nd = _criterion_inputs(70, 40, 7, 6, seed=1)
    out = []
    for _ in range(2):
        crit = PerVideoRewardCriterion()
        loss = crit(slp, seq, score, n=nd)
        (g,) = torch.autograd.grad(loss, slp)
        out.append((loss.detach().clone(), crit.last_advantage.clone(), g))
        torch.empty(1 << 16, device="cuda").fill_(float("nan"))      # what the next call's buffers may be carved from
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(out[1][0]))


def test_equal_scores_give_zero_advantages_and_zero_gradients():
    name = "mid_b3_s5"
    from controllable_xgating_amd import PerVideoRewardCriterion
    model = _model(name)
    a = _dev(name)
    seq, slp, n = model.rollout_per_video(*a[:4], uniforms=a[4])
    crit = PerVideoRewardCriterion()
    loss = crit(slp, seq, torch.full(seq.shape[:2], 0.5, device="cuda"), n=n)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.item()) == 0.0 and bool((crit.last_advantage == 0).all())
    for k, g in model_grads(model).items():
        assert (g == 0).all(), k


# ---- against the existing entry points
@pytest.mark.parametrize("name", ["mid_b3_s5", "tiny_s5", "rows_132"])
def test_eval_mode_tokens_equal_sample_per_video(name):
    model = _model(name, train=False)
    a = _dev(name)
    with torch.no_grad():
        seq, slp, n = model.rollout_per_video(*a[:4], uniforms=a[4])
        seq2, slp2, n2 = model.sample_per_video(*a[:4], {"sample_max": 0, "uniforms": a[4], "async": True})
    assert int(n.item()) == int(n2.item()) and torch.equal(seq, seq2)
    diff = float((slp - slp2).abs().max())
    print("%s: rollout_per_video vs sample_per_video: log-probs %s (max difference %.2e)"
          % (name, "bit-identical" if torch.equal(slp, slp2) else "not bit-identical", diff))
    assert diff <= 3e-4


def test_s1_against_sample_and_reward_criterion():
    """mid_s1: S = 1 with a given base is the reference's self-critical iteration: sample() + RewardCriterion + backward."""
    from controllable_xgating_amd import RewardCriterion
    name = "mid_s1"
    d, S, Pn, xv, pos, u = svo.case_inputs(name)
    score, base = _scores(name)
    ma, mb = _model(name), _model(name)
    seq_a, slp_a, loss_a, adv, k = _iteration(ma, name, "given")
    a = _dev(name)
    seq_b, slp_b = mb.sample(a[0], a[1], a[2], a[3].reshape(d.B, d.R), {"sample_max": 0, "uniforms": a[4]})
    loss_b = RewardCriterion()(slp_b, seq_b, torch.from_numpy(score - base[:, None]).cuda())
    loss_b.backward()
    torch.cuda.synchronize()
    assert np.array_equal(seq_a, seq_b.cpu().numpy())
    np.testing.assert_allclose(slp_a, slp_b.detach().cpu().numpy(), atol=3e-4)
    assert abs(loss_a - loss_b.item()) < 1e-4
    assert_grads_close(ma, model_grads(mb), skip=ZERO_GRAD_PARAMS)
    for x, y in zip((ma.two_spatial_encoder.visual_emb_rgb[1], ma.two_spatial_encoder.visual_emb_opfl[1]),
                    (mb.two_spatial_encoder.visual_emb_rgb[1], mb.two_spatial_encoder.visual_emb_opfl[1])):
        np.testing.assert_allclose(x.running_mean.cpu().numpy(), y.running_mean.cpu().numpy(), atol=1e-5)
        np.testing.assert_allclose(x.running_var.cpu().numpy(), y.running_var.cpu().numpy(), atol=1e-5)
        assert int(x.num_batches_tracked) == int(y.num_batches_tracked) == 1


@pytest.mark.parametrize("name", ["mid_b3_s5", "odd_s2", "rows_132"])
def test_nan_filled_workspace_changes_nothing(name):
    model = _model(name)
    _iteration(model, name)                                  # the first call allocates the workspace; the next ones reuse it
    ws = model._last_scst_video_ws[2]
    out = []
    for fill in (0, 255):                                    # 0xFF bytes: every float a NaN
        ws.fill_(fill)
        r = _iteration(model, name)
        assert model._last_scst_video_ws[2] is ws
        out.append(r + (model_grads(model),))
    (s0, l0, loss0, _, k0, g0), (s1, l1, loss1, _, k1, g1) = out
    assert k0 == k1 and np.array_equal(s0, s1) and np.isfinite(l1).all() and np.abs(l0 - l1).max() <= 1e-6 and abs(loss0 - loss1) <= 1e-6
    for n, g in g1.items():
        assert np.isfinite(g).all(), n
    assert_grads_close(model, g0, skip=ZERO_GRAD_PARAMS)


# ---- the Trainer
def _stub_scorer(rows, greedy):
    """A deterministic score per caption: the share of its words with an even id; M scores, or M + B with the greedy captions."""
    def share(c):
        return ((c > 0) & (c % 2 == 0)).sum(1) / np.maximum((c > 0).sum(1), 1)
    return share(rows) if greedy is None else np.concatenate([share(rows), share(greedy)])


def _trainer(model, S, baseline, overlap):
    from controllable_xgating_amd.driver import Trainer
    opt = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, overlap_update=overlap, learning_rate_decay_start=-1,
                             scheduled_sampling_start=-1, self_critical_after=0, scst_rows_per_video=S, scst_baseline=baseline)
    tr = Trainer(model, opt, reward_scorer=_stub_scorer)
    tr.start_epoch(0)
    assert tr.sc_flag
    return tr


@pytest.mark.parametrize("baseline", ["mean_others", "greedy"])
def test_trainer_two_iterations(baseline):
    name, S = "mid_b3_s5", 5
    d, _, Pn, xv, pos, u = svo.case_inputs(name)
    a = _dev(name)
    batch = dict(feat1=a[0], feat2=a[1], feat_mask=a[2], pos_feat=a[3][:, 0].contiguous())
    runs = []
    for overlap in (True, False):
        model = _model(name)
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        tr = _trainer(model, S, baseline, overlap)
        torch.manual_seed(7)
        infos = [tr.train_batch(batch) for _ in range(2)]
        torch.cuda.synchronize()
        assert all(np.isfinite(float(i["loss"].item())) and np.isfinite(i["avg_reward"]) for i in infos)
        assert tuple(tr.last_advantage.shape) == (d.B, S) and tr.iteration == 3
        if baseline == "mean_others":
            assert float(tr.last_advantage.sum(1).abs().max()) < 1e-5
        moved = sum(int((v.detach() != before[k]).any()) for k, v in model.named_parameters())
        assert moved > len(before) // 2
        bn = model.two_spatial_encoder.visual_emb_rgb[1]
        assert int(bn.num_batches_tracked) == (2 if baseline == "mean_others" else 4)      # the greedy rollout is a sample() call of its own
        runs.append(([float(i["loss"].item()) for i in infos], model))
    (la, ma), (lb, mb) = runs
    print("trainer %s: overlap %s, without %s" % (baseline, la, lb))
    np.testing.assert_allclose(la, lb, atol=2e-4)
    pb = dict(mb.named_parameters())
    for k, prm in ma.named_parameters():
        if k in ZERO_GRAD_PARAMS:
            continue
        np.testing.assert_allclose(prm.detach().cpu().numpy(), pb[k].detach().cpu().numpy(), atol=2e-5, err_msg=k)
    if baseline == "greedy":
        with pytest.raises(NotImplementedError):
            tr.train_batch(dict(batch, pos_feat=a[3]))


# ---- the raises and the workspace pool
def test_raises_and_workspace_pool():
    from controllable_xgating_amd import XgError
    from controllable_xgating_amd.model import _RolloutVideoFunction
    name = "tiny_s5"
    d, S, _, _, _, _ = svo.case_inputs(name)
    model = _model(name)
    a = _dev(name)
    with pytest.raises(ValueError):
        model.rollout_per_video(*a[:4], uniforms=a[4][:, 1:])
    with pytest.raises(ValueError):
        model.rollout_per_video(*a[:3], a[3].reshape(d.B * S, d.R))
    with pytest.raises(NotImplementedError):
        model.rollout_per_video(a[0].cpu(), *a[1:4])
    assert int(model.two_spatial_encoder.visual_emb_rgb[1].num_batches_tracked) == 0
    # without grad it runs and keeps nothing: one shared scratch, no graph
    with torch.no_grad():
        seq, slp, n = model.rollout_per_video(*a[:4], uniforms=a[4])
    assert not slp.requires_grad and [len(v) for (k, save), v in model._scst_video_pool.items() if save] in ([], [0])
    # a backward without saved activations: the library's error text
    seq, slp, n = _RolloutVideoFunction.apply(model, False, *a[:4], a[4], 1.0, *model._param_list())
    with pytest.raises(XgError, match="backward without saved activations"):
        slp.sum().backward()
    # with grad: the workspace is the call's own until the backward has run, then it returns to the pool and is reused
    seq, slp, n = model.rollout_per_video(*a[:4], uniforms=a[4])
    kept = [v for (k, save), v in model._scst_video_pool.items() if save]
    assert kept == [[]]
    slp.sum().backward()
    assert len(kept[0]) == 1
    ws = kept[0][0]
    seq2, slp2, _ = model.rollout_per_video(*a[:4], uniforms=a[4])
    assert kept[0] == [] and torch.equal(seq, seq2)
    slp2.sum().backward()
    assert kept[0][0] is ws
    # trim=True cuts both tensors to n
    seq3, slp3, n3 = model.rollout_per_video(*a[:4], uniforms=a[4], trim=True)
    assert seq3.shape[2] == slp3.shape[2] == int(n3.item()) and seq3.shape[:2] == (d.B, S)
    slp3.sum().backward()
