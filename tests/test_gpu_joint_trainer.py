"""JointTrainer on the MI355X (controllable_xgating_amd/joint.py; docs/JOINT_TRAINING.md): the joint iteration against the float64
composed oracle of tests/joint_oracle.py with the oracle's clip_adam, the detached form against two separate iterations, pure
caption-loss fine-tuning of the generator, the refusals and the checkpoint files.  Bounds: pos_train_oracle.traj_misses'."""
import argparse

import numpy as np
import pytest
import torch

from tests import joint_oracle as jo
from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, make_model

pytestmark = pytest.mark.gpu

LAM, LR, CLIP, STEPS = 0.5, pto.TRAJ_LR, pto.TRAJ_CLIP, 3
# gradients both models' existing backwards accumulate by float atomics (the embedding scatter-add, a2w.weight in the attention's post
# pass): two runs of the same iteration differ there in their last bits, so their parameters can differ in a last bit after Adam
ATOMIC_GRADS = ("embed.weight", "lstmcore.a2w.weight")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def _opt(**kw):
    o = argparse.Namespace(learning_rate=LR, weight_decay=0.0, grad_clip=CLIP, weight_class=WEIGHT_CLASS, learning_rate_decay_start=-1,
                           self_critical_after=-1, scheduled_sampling_start=-1, pos_loss_weight=LAM)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _models():
    from controllable_xgating_amd.pos import PosModel
    dc, dp, Pc, Pp, run, x = jo.joint_case()
    cap = make_model(dc, Pc)
    popt = argparse.Namespace(category_size=dp.C, input_encoding_size=dp.E, rnn_size=dp.R, att_size=dp.A, num_layers=1, drop_prob_lm=0.0,
                              seq_length=dp.L, feat_size=dp.F1, feat_size2=dp.F2)
    pos = PosModel(popt)
    pos.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(dp, Pp, run).items()}, strict=True)
    return cap, pos.cuda().train()


def _batch():
    x = jo.joint_case()[5]
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    return dict(feat1=t(x["feats_rgb"]), feat2=t(x["feats_opfl"]), feat_mask=t(x["feat_mask"]), cap=t(x["seq"]), cap_mask=t(x["seq_mask"]),
                cap_classes=t(x["cap_classes"]), class_mask=t(x["class_mask"]))


def _params(m):
    return {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}


def test_three_joint_iterations_against_the_float64_composed_oracle():
    from controllable_xgating_amd import JointTrainer
    dc, dp, Pc0, Pp0, run, x = jo.joint_case()
    gc, gp, losses = jo.joint_trajectory(LAM, STEPS, LR, CLIP)
    cap, pos = _models()
    tr = JointTrainer(cap, pos, _opt())
    tr.start_epoch(0)
    b = _batch()
    for it in range(STEPS):
        out = tr.train_batch(b)
        loss = float(out["loss"])
        print("iteration %d: loss %.6f (oracle %.6f), caption %.6f, tagging %.6f"
              % (it, loss, losses[it], float(out["loss_caption"]), float(out["loss_pos"])))
        assert abs(loss - losses[it]) < 1e-4
        assert abs(float(out["loss_caption"]) + LAM * float(out["loss_pos"]) - loss) < 1e-5
        torch.cuda.synchronize()
        miss = pto.traj_misses(_params(pos), Pp0, gp, it, LR)
        assert not miss, ("generator", it, miss)
        pc = {n: v for n, v in _params(cap).items() if n not in ZERO_GRAD_PARAMS}
        miss = pto.traj_misses(pc, Pc0, gc, it, LR)
        assert not miss, ("captioner", it, miss)
    assert tr.iteration == 1 + STEPS and tr.pos.iteration == 1 + STEPS
    # the path exists: the same three iterations with pos_feats detached end somewhere else
    cap2, pos2 = _models()
    tr2 = JointTrainer(cap2, pos2, _opt(joint_detach_pos=True))
    tr2.start_epoch(0)
    for _ in range(STEPS):
        tr2.train_batch(b)
    torch.cuda.synchronize()
    far = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(pos.parameters(), pos2.parameters()))
    assert far > 0.1 * LR, far


def test_detached_iteration_equals_two_separate_iterations_bit_for_bit():
    """joint_detach_pos with lambda = 1 (a weight of one leaves the generator's gradient as its own iteration forms it): both models'
    parameters after one iteration are those of one Trainer.train_batch -- on the vector the generator yields -- plus one
    PosTrainer.train_batch from the same start, bit for bit; the two parameters whose gradients the existing kernels sum by float
    atomics (ATOMIC_GRADS: not reproducible between two runs of the separate iterations either) within traj_misses' displacement
    bound, a tenth of the learning rate, for every element."""
    from controllable_xgating_amd import JointTrainer
    from controllable_xgating_amd.driver import Trainer
    from controllable_xgating_amd.pos_train import PosTrainer
    b = _batch()
    cap, pos = _models()
    tr = JointTrainer(cap, pos, _opt(pos_loss_weight=1.0, joint_detach_pos=True))
    tr.start_epoch(0)
    tr.train_batch(b)
    # the vector, from a generator of its own (its forward moves the running statistics)
    _, pos3 = _models()
    from controllable_xgating_amd.pos import prepare_pos_targets
    cap_r, new_mask = prepare_pos_targets(b["cap_classes"], b["class_mask"], check=False)
    with torch.no_grad():
        pos_feat = pos3(b["feat1"], b["feat2"], b["feat_mask"], None, None, cap_r, new_mask, return_pos_feats=True)[1].detach()
    cap2, pos2 = _models()
    t_cap, t_pos = Trainer(cap2, _opt()), PosTrainer(pos2, _opt())
    t_cap.start_epoch(0)
    t_pos.start_epoch(0)
    t_cap.train_batch(dict(b, pos_feat=pos_feat))
    t_pos.train_batch(b)
    torch.cuda.synchronize()
    for a, c, who in ((cap, cap2, "captioner"), (pos, pos2, "generator")):
        diff = [n for (n, p), q in zip(a.named_parameters(), c.parameters()) if n not in ATOMIC_GRADS and not torch.equal(p, q)]
        assert not diff, (who, diff)
        named = dict(c.named_parameters())
        for n in ATOMIC_GRADS:
            assert float((dict(a.named_parameters())[n] - named[n]).abs().max()) <= 0.1 * LR, (who, n)
        for (n, u), v in zip(a.named_buffers(), c.buffers()):
            assert torch.equal(u, v), (who, n)


def test_pos_loss_weight_zero_fine_tunes_the_generator_on_the_caption_loss_alone():
    from controllable_xgating_amd import JointTrainer
    cap, pos = _models()
    tr = JointTrainer(cap, pos, _opt(pos_loss_weight=0.0))
    tr.start_epoch(0)
    before = _params(pos)
    seen = {}
    step = tr.pos.optimizer.step

    def spy():
        torch.cuda.synchronize()
        seen.update({n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for n, p in pos.named_parameters()})
        step()

    tr.pos.optimizer.step = spy
    out = tr.train_batch(_batch())
    torch.cuda.synchronize()
    assert float(out["loss"]) == float(out["loss_caption"]) and np.isfinite(float(out["loss_pos"]))
    assert float(seen["logit.weight"].abs().max()) == 0.0 and float(seen["logit.bias"].abs().max()) == 0.0
    for n in ("lstmcore.lstmcell.h2h.weight", "lstmcore.lstmcell.a2h.weight", "lstmcore.lstmcell.i2h.weight"):
        assert float(seen[n].abs().max()) > 0, n
    after = _params(pos)
    assert np.array_equal(after["logit.weight"], before["logit.weight"]) and np.array_equal(after["logit.bias"], before["logit.bias"])
    assert not np.array_equal(after["lstmcore.lstmcell.h2h.weight"], before["lstmcore.lstmcell.h2h.weight"])
    # the gradient is the float64 oracle's at lambda = 0
    dc, dp, Pc, Pp, run, x = jo.joint_case()
    _, _, _, _, g64 = jo.joint_grads(Pc, Pp, run, x, dc, 0.0)
    miss = pto.golden_grad_misses({n: v.cpu().numpy() for n, v in seen.items()}, {"g/" + n: v for n, v in g64.items()})
    assert not miss, miss


def test_refusals():
    from controllable_xgating_amd import JointTrainer
    from controllable_xgating_amd.pos import PosModel
    cap, pos = _models()
    b = _batch()
    tr = JointTrainer(cap, pos, _opt())
    tr.start_epoch(0)
    q = dict(b, cap=b["cap"].unsqueeze(1).repeat(1, 2, 1), cap_mask=b["cap_mask"].unsqueeze(1).repeat(1, 2, 1))
    with pytest.raises(NotImplementedError, match=r"\(B,T\)"):
        tr.train_batch(q)
    dp = jo.joint_case()[1]
    other = PosModel(argparse.Namespace(category_size=dp.C, input_encoding_size=dp.E, rnn_size=dp.R + 8, att_size=dp.A, num_layers=1,
                                        drop_prob_lm=0.0, seq_length=dp.L, feat_size=dp.F1, feat_size2=dp.F2)).cuda()
    with pytest.raises(ValueError, match="rnn_size"):
        JointTrainer(cap, other, _opt())
    sc = JointTrainer(cap, pos, _opt(self_critical_after=0))
    with pytest.raises(NotImplementedError, match="self-critical"):
        sc.start_epoch(0)
    with pytest.raises(NotImplementedError, match="self-critical"):
        sc.train_batch(b)
    # nothing moved: a refused call takes no step
    assert tr.iteration == 1


def test_one_directory_holds_both_checkpoints(tmp_path):
    import os
    from controllable_xgating_amd import JointTrainer
    cap, pos = _models()
    tr = JointTrainer(cap, pos, _opt())
    tr.start_epoch(0)
    tr.train_batch(_batch())
    path = str(tmp_path / "ckpt")
    tr.save_checkpoint(path, 0.25)
    assert not tr.update_best(path, 0.5) and not tr.update_best(path, 0.4)
    assert sorted(os.listdir(path)) == ["infos-best.pkl", "infos-pos-best.pkl", "infos-pos.pkl", "infos.pkl", "model-best.pth",
                                        "model-pos-best.pth", "model-pos.pth", "model.pth"]
    cap2, pos2 = _models()
    infos, pinfos = JointTrainer.resume(cap2, pos2, path)
    assert infos["iter"] == 2 and pinfos["iter"] == 2 and infos["val_score"] == 0.5
    for a, c in ((cap, cap2), (pos, pos2)):
        sa, sc = a.state_dict(), c.state_dict()
        assert list(sa) == list(sc) and all(torch.equal(sa[k].cpu(), sc[k].cpu()) for k in sa)
