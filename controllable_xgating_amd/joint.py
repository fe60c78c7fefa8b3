"""Joint training of the captioner and the POS sequence generator (docs/JOINT_TRAINING.md): one iteration in which the
generator's train-mode forward produces the global POS vector the captioner consumes, the caption loss's gradient with respect to
that vector flows back into the generator, and both models step.  The reference trains the two stages one after the other
(pos_src/starttrain_trainpos.py, then caption_src/starttrain.py on the extracted vectors); this is the step it has no script for.

``JointTrainer`` holds a ``driver.Trainer`` and a ``pos_train.PosTrainer`` -- two ``ClipAdam`` s, two learning-rate schedules --
and runs ``loss = L_cap + opt.pos_loss_weight * L_pos`` through ONE ``loss.backward()``; autograd orders the captioner's HIP
backward, the sum that forms d L_cap / d pos_feats and the generator's HIP backward.  Data loading is out of scope, as in both
trainers: batches are dicts of CUDA tensors."""
from __future__ import annotations

import os

import torch

from .driver import Trainer
from .pos_train import PosTrainer

POS_TAG = "-pos"                        # the generator's checkpoint files in the shared directory: model-pos<tag>.pth, infos-pos<tag>.pkl


class JointTrainer:
    """``JointTrainer(cap_model, pos_model, opt, reward_scorer=None)``.

    Options read from ``opt`` besides the two trainers' own: ``pos_loss_weight`` (lambda, default 1.0; 0 = the generator is
    fine-tuned on the caption loss alone and its backward receives no gradient for its log-probabilities) and
    ``joint_detach_pos`` (default False; True cuts the path, so both models receive exactly the gradients of two separate
    iterations).  ``pos_opt``: a second options object for the generator's trainer (learning rate, decay, clip); default ``opt``."""

    def __init__(self, cap_model, pos_model, opt, reward_scorer=None, pos_opt=None):
        if int(cap_model.rnn_size) != int(pos_model.rnn_size):
            raise ValueError("the captioner's rnn_size (%d) and the POS generator's (%d) must agree: the generator's state is the "
                             "captioner's pos_feats" % (cap_model.rnn_size, pos_model.rnn_size))
        self.opt = opt
        self.cap = Trainer(cap_model, opt, reward_scorer)
        self.pos = PosTrainer(pos_model, opt if pos_opt is None else pos_opt)
        if self.cap.grad_sync is not None:
            raise NotImplementedError("joint training is single-process: the data-parallel gradient exchange covers the captioner only")
        if not self.cap.fused:
            raise NotImplementedError("joint training runs the fused caption loss (fused_xe_loss): the un-fused model() path "
                                      "returns no gradient for pos_feats")

    @property
    def iteration(self):
        return self.cap.iteration

    def start_epoch(self, epoch):
        """Both trainers' schedules (learning rates, the captioner's ss_prob).  A self-critical epoch is refused: the gradient
        through SCST rollouts is not implemented."""
        self.cap.start_epoch(epoch)
        self.pos.start_epoch(epoch)
        if self.cap.sc_flag:
            raise NotImplementedError("joint training has no self-critical form: epoch %d sets sc_flag (self_critical_after)" % epoch)

    def train_batch(self, b):
        """One joint iteration.  b: the union of the two trainers' batch keys -- feat1, feat2, feat_mask, cap (B,T), cap_mask,
        cap_classes, class_mask; a pos_feat entry is not read (the generator supplies it).  Returns a dict: loss, loss_caption,
        loss_pos (device scalars).  One host synchronisation: the generator's forward reads T'."""
        cap_tr, pos_tr, opt = self.cap, self.pos, self.opt
        if cap_tr.sc_flag:
            raise NotImplementedError("joint training has no self-critical form (sc_flag is set)")
        if b["cap"].dim() != 2:
            raise NotImplementedError("joint training needs a (B,T) batch: the POS generator has no rows-per-video training form, "
                                      "got cap %s" % (tuple(b["cap"].shape),))
        cap_model, pos_model = cap_tr.model, pos_tr.model
        lam = float(getattr(opt, "pos_loss_weight", 1.0))
        cap_r, new_mask = pos_tr._targets(b, b["feat_mask"].device)
        mask = b.get("cap_mask", new_mask)
        cap_tr.optimizer.zero_grad()
        pos_tr.optimizer.zero_grad()
        # the generator on the batch's reference tags: its log-probabilities and the state the captioner consumes
        logp, pos_feats = pos_model(b["feat1"], b["feat2"], b["feat_mask"], None, None, cap_r, new_mask, return_pos_feats=True)
        if getattr(opt, "joint_detach_pos", False):
            pos_feats = pos_feats.detach()
        class_mask = torch.as_tensor(b["class_mask"]).to(logp.device)
        # lambda = 0: the tagging loss is reported only, and the generator's backward gets no gradient for logp (none is built)
        loss_pos = pos_tr.classify_crit(logp if lam != 0.0 else logp.detach(), cap_r, mask, class_mask)
        wc = getattr(opt, "weight_class", 0.0)
        ss = bool(cap_model.training and cap_model.ss_prob > 0.0)
        if ss and not (getattr(opt, "fused_ss_loss", True) and getattr(cap_model, "precision", "fp32") == "fp32"):
            raise NotImplementedError("joint training under scheduled sampling needs the fused fp32 loss (fused_ss_loss)")
        xe = cap_model.xe_loss_ss if ss else cap_model.xe_loss
        loss_cap = xe(b["feat1"], b["feat2"], b["feat_mask"], pos_feats, b["cap"], b["cap_mask"], b.get("cap_classes"),
                      b.get("class_mask"), wc)
        loss = loss_cap + lam * loss_pos if lam != 0.0 else loss_cap
        cap_tr.optimizer.arm()                        # (the captioner's update overlaps its backward's tail, as in Trainer)
        loss.backward()
        cap_tr.optimizer.step()
        pos_tr.optimizer.step()
        cap_tr.iteration += 1
        pos_tr.iteration += 1
        return dict(loss=loss.detach(), loss_caption=loss_cap.detach(), loss_pos=loss_pos.detach())

    # ------------------------------------------------------------ checkpoints: one directory, the two trainers' files
    def save_checkpoint(self, path, val_score=None, tag=""):
        """model<tag>.pth / infos<tag>.pkl (the captioner's, Trainer.save_checkpoint) and model-pos<tag>.pth / infos-pos<tag>.pkl
        (the generator's, PosTrainer.save_checkpoint) in `path`."""
        self.cap.save_checkpoint(path, val_score, tag)
        self.pos.save_checkpoint(path, val_score, POS_TAG + tag)

    def update_best(self, path, current_score):
        """Trainer.update_best on the captioner's validation score; the generator that produced it is saved beside it.  Returns
        True when training should stop."""
        before = self.cap.best_val_score
        stop = self.cap.update_best(path, current_score)
        if self.cap.best_val_score != before:
            self.pos.best_val_score = self.cap.best_val_score
            self.pos.save_checkpoint(path, current_score, POS_TAG + "-best")
        return stop

    @staticmethod
    def resume(cap_model, pos_model, path, tag="-best", strict=True):
        """Both state_dicts from `path`; returns (captioner infos, generator infos)."""
        infos = Trainer.resume(cap_model, path, tag, strict)
        pos_model.load_state_dict(torch.load(os.path.join(path, "model%s%s.pth" % (POS_TAG, tag))), strict=strict)
        return infos, torch.load(os.path.join(path, "infos%s%s.pkl" % (POS_TAG, tag)), weights_only=False)
