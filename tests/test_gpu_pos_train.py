"""Training the POS sequence generator on the MI355X: PosModel's train-mode HIP forward and backward against the reference's own
train-mode outputs (tests/golden/pos_train_*.npz, p = 0 and the hash-mask p = 0.5 case), against tests/pos_train_oracle.py at
p = 0.5 (mid and full size), the three-iteration PosModel + ClipAdam trajectory against the reference's Adam, gradient
accumulation, eval after training, T' < T and the stale-activation guard."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import ROOT, grad_misses

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def make_opt(d, p):
    return argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1, drop_prob_lm=p,
                              seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)


def pos_model(d, P, run, p=0.0, seed=0):
    from controllable_xgating_amd.pos import PosModel
    m = PosModel(make_opt(d, p))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    m = m.cuda().train()
    m.dropout_seed = seed
    return m


def batch(x):
    from controllable_xgating_amd.pos import prepare_pos_targets
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = prepare_pos_targets(torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"]))
    return fr, fo, fm, cap_r.cuda(), new_mask.cuda(), torch.from_numpy(x["class_mask"]).cuda()


def train_step(m, x):
    """forward + ClassiferCriterion + backward; returns (loss, logp)."""
    from controllable_xgating_amd.pos import ClassiferCriterion
    fr, fo, fm, cap_r, new_mask, cm = batch(x)
    out = m(fr, fo, fm, None, None, cap_r, new_mask)
    loss = ClassiferCriterion()(out, cap_r, new_mask, cm)
    loss.backward()
    return loss.item(), out.detach()


def grads_of(m):
    return {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy() for n, p in m.named_parameters()}


def running_of(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if "running" in k}


@pytest.mark.parametrize("name", list(pto.TRAIN_CASES))
def test_hip_train_step_matches_reference_goldens(name):
    cfg, kw, p, seed = pto.TRAIN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, **kw)
    g = dict(np.load(os.path.join(GOLD, "pos_train_%s.npz" % name)))
    m = pos_model(d, P, run, p, seed)
    loss, out = train_step(m, x)
    assert out.shape[1] == int(g["tf_T"])
    assert abs(loss - float(g["loss"])) < 1e-4
    miss = pto.golden_grad_misses(grads_of(m), g, rtol=2e-3, atol=2e-6, zero_atol=1e-5)
    assert not miss, miss
    rs = running_of(m)
    for mo in ("rgb", "opfl"):
        for b in ("running_mean", "running_var"):
            np.testing.assert_allclose(rs["two_fc_encoder.visual_emb_%s.1.%s" % (mo, b)], g["run/%s/%s" % (mo, b)], rtol=1e-4, atol=1e-5)
    assert int(m.two_fc_encoder.visual_emb_rgb[1].num_batches_tracked) == 1


def test_tfzero_stops_at_the_all_zero_column():
    cfg, kw, p, seed = pto.TRAIN_CASES["tfzero"]
    d = po.make_dims(**po.POS_CFG[cfg])
    x = po.make_inputs(d, **kw)
    m = pos_model(d, po.make_params(d), po.make_running(d))
    _, out = train_step(m, x)
    assert out.shape[1] < d.L + 1
    assert out.shape[1] == int(np.load(os.path.join(GOLD, "pos_train_tfzero.npz"))["tf_T"])


@pytest.mark.parametrize("cfg", ["mid", "full64"])
def test_hip_matches_train_oracle_with_dropout(cfg):
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, seed=6, ragged=True)
    seed = 4321
    m = pos_model(d, P, run, 0.5, seed)
    loss, out = train_step(m, x)
    # the reference: the oracle in float64 on the same GPU (eager torch)
    lo, go, _, ro, out_o = pto.loss_and_grads(d, P, run, x, 0.5, seed, dtype=torch.float64, device="cuda")
    assert abs(loss - lo) < 1e-4 * max(1.0, abs(lo))
    np.testing.assert_allclose(out.cpu().numpy(), out_o, atol=3e-4)
    gh = grads_of(m)
    miss = grad_misses(gh, go, skip=pto.ZERO_GRAD)
    assert not miss, miss
    for n in pto.ZERO_GRAD:
        assert np.abs(gh[n]).max() < 1e-5, n
    rs = running_of(m)
    for k, v in ro.items():
        np.testing.assert_allclose(rs[k], v, rtol=1e-4, atol=1e-5)


def test_two_backwards_without_zero_grad_give_twice_the_gradient():
    d = po.make_dims(**po.POS_CFG["mid"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=2, ragged=True)
    m = pos_model(d, P, run, 0.5, 99)
    m.flat_grads().zero_()                          # every p.grad bound to the flat buffer: the library adds into it
    train_step(m, x)
    g1 = grads_of(m)
    train_step(m, x)                                # same seed: same masks; the running statistics moved, the batch ones did not
    g2 = grads_of(m)
    for n in g1:
        np.testing.assert_allclose(g2[n], 2 * g1[n], rtol=1e-4, atol=1e-6 + 1e-4 * np.abs(g1[n]).max(), err_msg=n)
    # and through autograd's own accumulation (p.grad not bound to the flat buffer)
    m2 = pos_model(d, P, run, 0.5, 99)
    train_step(m2, x)
    train_step(m2, x)
    for n, v in grads_of(m2).items():
        np.testing.assert_allclose(v, g2[n], rtol=1e-4, atol=1e-6 + 1e-4 * np.abs(g2[n]).max(), err_msg=n)


def test_stale_activations_backward_raises():
    from controllable_xgating_amd import XgError
    from controllable_xgating_amd.pos import ClassiferCriterion
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = pos_model(d, po.make_params(d), po.make_running(d))
    fr, fo, fm, cap_r, new_mask, cm = batch(po.make_inputs(d, seed=0))
    out1 = m(fr, fo, fm, None, None, cap_r, new_mask)
    out2 = m(fr, fo, fm, None, None, cap_r, new_mask)
    with pytest.raises(XgError, match="overwritten"):
        ClassiferCriterion()(out1, cap_r, new_mask, cm).backward()
    ClassiferCriterion()(out2, cap_r, new_mask, cm).backward()      # the latest one still works


def test_trajectory_posmodel_clipadam_vs_reference_adam_golden():
    from controllable_xgating_amd.pos_train import PosTrainer
    cfg, kw = pto.TRAJ_CASE
    d = po.make_dims(**po.POS_CFG[cfg])
    P0, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, **kw)
    g = dict(np.load(os.path.join(GOLD, "pos_train_traj.npz")))
    m = pos_model(d, P0, run)
    opt = argparse.Namespace(learning_rate=pto.TRAJ_LR, grad_clip=pto.TRAJ_CLIP, learning_rate_decay_start=-1)
    tr = PosTrainer(m, opt)
    tr.start_epoch(0)
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    b = dict(feat1=fr, feat2=fo, feat_mask=fm, cap_classes=torch.from_numpy(x["cap_classes"]).cuda(),
             class_mask=torch.from_numpy(x["class_mask"]).cuda())
    for it in range(pto.TRAJ_STEPS):
        loss = tr.train_batch(b).item()
        assert abs(loss - g["losses"][it]) < 1e-4
        Pn = {n: p.detach().cpu().numpy() for n, p in m.named_parameters()}
        miss = pto.traj_misses(Pn, P0, g, it)
        assert not miss, (it, miss)


def test_eval_after_training_matches_pos_oracle():
    """After two training steps, eval-mode forward and greedy sample read the updated weights and running statistics."""
    from controllable_xgating_amd.pos_train import PosTrainer
    d = po.make_dims(**po.POS_CFG["mid"])
    P0, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, seed=2, ragged=True)
    m = pos_model(d, P0, run, 0.5, 7)
    tr = PosTrainer(m, argparse.Namespace(learning_rate=1e-3, grad_clip=0.1, learning_rate_decay_start=-1))
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    b = dict(feat1=fr, feat2=fo, feat_mask=fm, cap_classes=torch.from_numpy(x["cap_classes"]).cuda(),
             class_mask=torch.from_numpy(x["class_mask"]).cuda())
    for _ in range(2):
        tr.train_batch(b)
    assert int(m.two_fc_encoder.visual_emb_opfl[1].num_batches_tracked) == 2
    val = tr.validate([b])
    m.eval()
    Pn = {n: p.detach().cpu().numpy() for n, p in m.named_parameters()}
    rn = {k: v for k, v in running_of(m).items()}
    Pt, rt = po.to_torch(Pn), po.to_torch(rn)
    fr_c, fo_c, fm_c = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    out_o = po.forward_tf(Pt, rt, fr_c, fo_c, fm_c, cap_r, new_mask)
    loss_o = float(po.criterion(out_o, cap_r, new_mask, torch.from_numpy(x["class_mask"])))
    assert abs(val - loss_o) < 1e-4
    with torch.no_grad():
        out = m(fr, fo, fm, None, None, cap_r.cuda(), new_mask.cuda())
        seq, slp, states, masks = m.sample(fr, fo, fm, {"sample_max": 1})
    np.testing.assert_allclose(out.cpu().numpy(), out_o.numpy(), atol=3e-4)
    so, slo, sto, mo, lps = po.sample_greedy(Pt, rt, fr_c, fo_c, fm_c, d.L)
    top2 = torch.topk(lps, 2, dim=2).values
    margin = (top2[..., 0] - top2[..., 1]).numpy()
    n = min(seq.shape[1], so.shape[1])
    ok = margin[:n].T >= 1e-3                       # (B, n): choices that are not near-ties
    first_tie = np.where(~ok.all(0))[0]
    k = int(first_tie[0]) if first_tie.size else n
    np.testing.assert_array_equal(seq.cpu().numpy()[:, :k], so.numpy()[:, :k])
    np.testing.assert_allclose(states.cpu().numpy()[:, :k + 1], sto.numpy()[:, :k + 1], atol=1e-4)


def test_trainer_host_or_device_class_mask_and_validate_keeps_the_mode():
    """train_batch takes class_mask on the host (checked there) or on the device (no extra synchronisation): same loss;
    validate() leaves the model in the mode it found it in."""
    from controllable_xgating_amd.pos_train import PosTrainer
    d = po.make_dims(**po.POS_CFG["mid"])
    P0, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, seed=2, ragged=True)
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    losses = []
    for dev in ("cpu", "cuda"):
        m = pos_model(d, P0, run, 0.5, 11)
        tr = PosTrainer(m, argparse.Namespace(learning_rate=1e-3, grad_clip=0.1, learning_rate_decay_start=-1))
        b = dict(feat1=fr, feat2=fo, feat_mask=fm, cap_classes=torch.from_numpy(x["cap_classes"]).to(dev),
                 class_mask=torch.from_numpy(x["class_mask"]).to(dev))
        losses.append(tr.train_batch(b).item())
        tr.validate([b])
        assert m.training
        m.eval()
        v = tr.validate([b])
        assert not m.training and np.isfinite(v)
    assert losses[0] == losses[1]
