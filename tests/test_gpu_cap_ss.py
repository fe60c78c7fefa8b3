"""The fused teacher-forced loss under scheduled sampling on the MI355X: SAModel.xe_loss_ss and xe_loss_ss_per_video
(include/xgate_ss.h) against the oracle of tests/cap_ss_oracle.py.

Per case: (1) the fed tokens against the oracle's own draw from the same uniforms -- rows equal, except a row whose first difference
is a draw whose u_tok lies within 3e-4 of an edge of the oracle's float64 CDF interval, at most two rows per case; (2) the float64
oracle replays the kernel's fed tokens: loss and both criteria within 1e-4, every parameter gradient by grad_misses at its defaults
(under the ReLU-flip exemptions of oracle_f64_with_flips), running statistics within 1e-5 against one update from the B videos.
The cases and what each reaches: tests/cap_ss_oracle.py, checked without a GPU in tests/test_cap_ss_cpu.py."""
import argparse
import functools

import numpy as np
import pytest
import torch

from oracle import xgate_oracle as xo
from tests import cap_ss_oracle as sso
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, grad_misses, make_model, model_grads, oracle_f64_with_flips

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The device inputs of a case in the order its method takes them (made once, shared, never changed)."""
    d, Q, _, x, _, _ = sso.case_inputs(name)
    T = d.L + 1
    cls = sso.CASES[name][3]
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    rows = lambda a: t(a) if Q == 0 else t(a).reshape(d.B, Q, *a.shape[1:])      # noqa: E731
    del T
    return (t(x["feats_rgb"]), t(x["feats_opfl"]), t(x["feat_mask"]), rows(x["pos_feats"]), rows(x["seq"]), rows(x["seq_mask"]),
            rows(x["cap_classes"]) if cls else None, rows(x["class_mask"]) if cls else None, WEIGHT_CLASS if cls else 0.0)


def _model(name, train=True, ss=True):
    d, Q, P, _, u_sel, u_tok = sso.case_inputs(name)
    p = sso.CASES[name][5]
    m = make_model(d, P, p_drop=p, train=train)
    if p > 0:
        m.dropout_seed = sso.DROP_SEED
    m.ss_prob = sso.CASES[name][4] if ss else 0.0
    m.ss_uniforms = (torch.from_numpy(u_sel).cuda(), torch.from_numpy(u_tok).cuda())
    return m


def _call(model, name):
    Q = sso.CASES[name][2]
    return (model.xe_loss_ss if Q == 0 else model.xe_loss_ss_per_video)(*_dev(name))


def _step(model, name):
    """loss.backward() of one call; returns (loss, last_losses, fed tokens (T, M) ndarray)."""
    model.zero_grad(set_to_none=True)
    loss = _call(model, name)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), model.last_losses.cpu().numpy(), model.last_ss_tokens.cpu().numpy()


@pytest.mark.parametrize("name", sorted(sso.CASES))
def test_fed_tokens_loss_gradients_and_running_statistics_vs_oracle(name):
    d, Q, P, x, u_sel, u_tok = sso.case_inputs(name)
    ss_prob = sso.CASES[name][4]
    model = _model(name)
    loss, ll, tok = _step(model, name)
    assert tok.shape == (d.L + 1, sso.rows_of(name)) and tok.dtype == np.int64
    # (1) the kernel's fed tokens against the oracle's own draw
    tok_o, logp_o = sso.case_draw(name)
    excused = sso.assert_fed_tokens_match(tok, tok_o, logp_o, x["seq"], u_sel, u_tok, ss_prob)
    coin = u_sel < ss_prob
    coin[0] = False
    print("%s: %d of %d (t, m) draw, %d fed tokens differ from seq, rows excused %s"
          % (name, int(coin.sum()), coin.size, int((tok != x["seq"].T).sum()), excused))
    assert np.array_equal(tok[~coin], x["seq"].T[~coin])
    # (2) the float64 oracle replays the kernel's fed tokens
    loss_o, (lm_o, lc_o, running), g64, ex = oracle_f64_with_flips(P, x, sso.replay_fn(name, tok))
    print("%s: loss %.6f (oracle %.6f), lm %.6f (%.6f), cls %.6f (%.6f)" % (name, loss, loss_o, ll[1], lm_o, ll[2], lc_o))
    assert abs(loss - loss_o) < 1e-4 and abs(ll[0] - loss_o) < 1e-4
    assert abs(ll[1] - lm_o) < 1e-4 and abs(ll[2] - lc_o) < 1e-4
    report = {}
    bad = grad_misses(model_grads(model), g64, skip=ZERO_GRAD_PARAMS, exempt=ex, report=report)
    print("%s: worst gradient %s" % (name, max(report.items(), key=lambda kv: kv[1][2])))
    assert not bad, bad
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), running[pre + "running_mean"].numpy(), atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), running[pre + "running_var"].numpy(), atol=1e-5)
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("name", ["mid", "v_mid_q5"])
@pytest.mark.parametrize("how", ["eval", "ss_prob_0"])
def test_eval_mode_and_ss_prob_zero_equal_the_teacher_forced_loss_bit_for_bit(name, how):
    """Eval mode at ss_prob 0.5, and train mode at ss_prob 0: the methods call xe_loss / xe_loss_per_video themselves and hand on
    what those return.  Two separate runs of xe_loss differ in their last bits (its cross-entropy rows add into the sums by float
    atomics), so "bit for bit" is checked against the sibling's own return value of that call, recorded by a wrapper; a second
    model's separate xe_loss run is compared within ten units in the last place besides."""
    Q = sso.CASES[name][2]
    train = how != "eval"
    a, b = _model(name, train=train, ss=not train), _model(name, train=train, ss=False)
    sibling = "xe_loss" if Q == 0 else "xe_loss_per_video"
    inner, seen = getattr(a, sibling), []

    def spy(*args, **kw):
        if not train:
            assert a.ss_prob > 0
        out = inner(*args, **kw)
        seen.append((out.clone(), a.last_losses.clone()))
        return out

    setattr(a, sibling, spy)
    with torch.no_grad():
        la = _call(a, name)
        lb = getattr(b, sibling)(*_dev(name))
    torch.cuda.synchronize()
    assert len(seen) == 1 and torch.equal(la, seen[0][0]) and torch.equal(a.last_losses, seen[0][1])
    # (ten units in the last place of a float32 below 8: 4.8e-7 each)
    assert abs(float(la) - float(lb)) <= 5e-6 and float((a.last_losses - b.last_losses).abs().max()) <= 5e-6
    seq = _dev(name)[4]
    assert torch.equal(a.last_ss_tokens, seq.reshape(-1, seq.shape[-1]).t())


@pytest.mark.parametrize("name", ["mid", "mid_b132", "v_mid_q5"])
def test_two_identical_calls_feed_identical_tokens(name):
    a, b = _model(name), _model(name)
    la, _, ta = _step(a, name)
    lb, _, tb = _step(b, name)
    assert np.array_equal(ta, tb) and abs(la - lb) <= 5e-6      # (the sums' float atomics: ten units in the last place)
    x = sso.case_inputs(name)[3]
    assert (ta != x["seq"].T).any()


@pytest.mark.parametrize("name", ["mid", "odd", "v_mid_q5"])
def test_nan_filled_workspace_gives_the_same_result(name):
    """Everything but the step's synchronisation words (they are zero between launches by contract: xg_workspace_init) is NaN."""
    model = _model(name)
    _step(model, name)                                       # the first call allocates the workspace; the next ones reuse it
    ws = model._last_ss_ws
    out = []
    for fill in (0, 255):                                    # 0xFF bytes: every float a NaN
        ws.fill_(fill)
        out.append(_step(model, name) + (model_grads(model),))
        assert model._last_ss_ws is ws
    (l0, ll0, t0, g0), (l1, ll1, t1, g1) = out
    assert np.isfinite(l1) and abs(l0 - l1) <= 5e-6 and np.abs(ll0 - ll1).max() <= 5e-6 and np.array_equal(t0, t1)
    for n, g in g1.items():
        assert np.isfinite(g).all(), n
    bad = grad_misses(g1, g0, skip=ZERO_GRAD_PARAMS)
    assert not bad, bad


def test_xe_loss_ss_vs_the_unfused_forward_under_the_same_uniforms():
    """mid: model() + LanguageModelCriterion (xg_forward_ss) under the same ss_uniforms.  Both draw by the same rule, each from its own
    logits.  At drop_prob_lm 0 a row's log-probs depend on its own fed tokens only (the encoder sees the same batch), so the loss
    over the rows whose fed tokens agree -- every other row's seq_mask zeroed in both -- is compared within 1e-4."""
    from controllable_xgating_amd import LanguageModelCriterion
    name = "mid"
    a, b = _model(name), _model(name)
    args = _dev(name)[:6]
    with torch.no_grad():
        a.xe_loss_ss(*args)
        logp, _ = b(*args)
    tok = a.last_ss_tokens.cpu().numpy()
    # the un-fused path's fed tokens: the rule applied to ITS log-probs
    u_sel, u_tok = (u.cpu().numpy() for u in a.ss_uniforms)
    seq, lp = args[4].cpu().numpy(), logp.cpu().numpy()
    fed = seq.T.copy()
    for t in range(1, seq.shape[1]):
        for m in range(seq.shape[0]):
            if u_sel[t, m] < a.ss_prob:
                fed[t, m] = xo.sample_token(lp[m, t - 1], float(u_tok[t, m]))
    same = (fed == tok).all(0)
    assert same.sum() >= same.size - sso.MAX_EXCUSED_ROWS, np.flatnonzero(~same)
    mask = args[5] * torch.from_numpy(same.astype(np.float32)).cuda().unsqueeze(1)
    with torch.no_grad():
        la = float(_model(name).xe_loss_ss(*args[:5], mask).item())
        lb = float(LanguageModelCriterion()(logp, args[4], mask).item())
    print("un-fused %.6f, fused %.6f over the %d of %d rows that feed the same tokens" % (lb, la, int(same.sum()), same.size))
    assert abs(la - lb) < 1e-4, (la, lb)


def _trainer(model, overlap=True):
    from controllable_xgating_amd.driver import Trainer
    opt = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, weight_class=WEIGHT_CLASS, overlap_update=overlap,
                             learning_rate_decay_start=-1, self_critical_after=-1, scheduled_sampling_start=0,
                             scheduled_sampling_increase_every=1, scheduled_sampling_increase_prob=0.05, scheduled_sampling_max_prob=0.25)
    tr = Trainer(model, opt)
    tr.start_epoch(5)                       # five increases of 0.05: the maximum of the reference's recipe
    assert model.ss_prob == 0.25
    return tr


@pytest.mark.parametrize("name", ["mid", "v_mid_q5"])
@pytest.mark.parametrize("overlap", [True, False])
def test_trainer_two_iterations_at_ss_prob_025_through_the_schedule(name, overlap):
    model = _model(name)
    model.ss_uniforms = None                # fresh uniforms per iteration, as training draws them
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    tr = _trainer(model, overlap)
    a = _dev(name)
    batch = dict(feat1=a[0], feat2=a[1], feat_mask=a[2], pos_feat=a[3], cap=a[4], cap_mask=a[5], cap_classes=a[6], class_mask=a[7])
    cap = a[4].reshape(-1, a[4].shape[-1]).t()
    for _ in range(2):
        loss = float(tr.train_batch(batch)["loss"].item())
        assert np.isfinite(loss)
        assert model.last_ss_tokens.shape == cap.shape and bool((model.last_ss_tokens != cap).any())
    torch.cuda.synchronize()
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) >= len(before) - len(ZERO_GRAD_PARAMS), sorted(set(before) - set(moved))


def test_trainer_refuses_per_video_batches_without_the_fused_loss():
    name = "v_mid_q5"
    model = _model(name)
    tr = _trainer(model)
    tr.opt.fused_ss_loss = False
    a = _dev(name)
    batch = dict(feat1=a[0], feat2=a[1], feat_mask=a[2], pos_feat=a[3], cap=a[4], cap_mask=a[5], cap_classes=a[6], class_mask=a[7])
    with pytest.raises(NotImplementedError):
        tr.train_batch(batch)
    with pytest.raises(NotImplementedError):
        model.xe_loss_per_video(*a)         # the teacher-forced per-video loss keeps its refusal
    model.ss_uniforms = (model.ss_uniforms[0][:, 1:], model.ss_uniforms[1])
    with pytest.raises(ValueError):
        model.xe_loss_ss_per_video(*a)
