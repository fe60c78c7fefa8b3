"""Training driver of the POS sequence generator: the call sequence of the reference's pos_src/starttrain_trainpos.py:84-238
(teacher forcing only -- its self-critical branch exits) on top of ``pos.PosModel``.  Data loading and TensorBoard are out of scope:
batches are handed in as dicts of CUDA tensors, as the reference's collate_fn yields them.  ``pos.extract_pos_features`` on the
trained model is the hand-off to the captioner."""
from __future__ import annotations

import os

import torch

from .driver import lr_for_epoch
from .pos import ClassiferCriterion, prepare_pos_targets
from .train import ClipAdam


class PosTrainer:
    """One object = the body of the reference's POS training loop without the data loader."""

    def __init__(self, model, opt):
        self.model, self.opt = model, opt
        self.classify_crit = ClassiferCriterion()
        self.optimizer = ClipAdam(model, lr=opt.learning_rate, weight_decay=getattr(opt, "weight_decay", 0.0),
                                  grad_clip=getattr(opt, "grad_clip", 0.1))
        self.iteration, self.epoch = 1, 0
        self.best_val_score = None
        self.patience = 0

    def start_epoch(self, epoch):
        """the update_lr_flag block, starttrain_trainpos.py:94-115 (step decay of the learning rate; the POS model ignores
        ss_prob and the self-critical branch is not run)."""
        self.epoch = epoch
        self.opt.current_lr = lr_for_epoch(self.opt, epoch)
        self.optimizer.set_lr(self.opt.current_lr)

    @staticmethod
    def _targets(b, device):
        """prepare_pos_targets without a host synchronisation: a class_mask still on the host (as the collate_fn yields it) is
        checked there for free and the targets are copied over; one already on the device is not re-checked (a row without a
        non-zero entry then gets new_mask all ones), so that the iteration's one synchronisation stays the read of T'."""
        cm = torch.as_tensor(b["class_mask"])
        if cm.is_cuda:
            return prepare_pos_targets(b["cap_classes"], cm, check=False)
        cap_r, new_mask = prepare_pos_targets(torch.as_tensor(b["cap_classes"]).cpu(), cm)
        if torch.device(device).type == "cuda":          # (pinned: the copies do not wait for the stream)
            cap_r, new_mask = cap_r.pin_memory(), new_mask.pin_memory()
        return cap_r.to(device, non_blocking=True), new_mask.to(device, non_blocking=True)

    def train_batch(self, b):
        """starttrain_trainpos.py:130-152.  b: dict with feat1, feat2, feat_mask, cap_classes (as collated, not rolled),
        class_mask and optionally cap_mask (the criterion's mask; new_mask when absent).  Returns the loss (a device scalar).
        One host synchronisation: the forward's read of T'."""
        model = self.model
        cap_r, new_mask = self._targets(b, b["feat_mask"].device)
        mask = b.get("cap_mask", new_mask)
        self.optimizer.zero_grad()                                                                    # :138
        out = model(b["feat1"], b["feat2"], b["feat_mask"], None, None, cap_r, new_mask)               # :141
        loss = self.classify_crit(out, cap_r, mask, torch.as_tensor(b["class_mask"]).to(out.device))  # :142
        loss.backward()                                                                               # :150
        self.optimizer.step()                                                                         # :151-152 (clamp + Adam)
        self.iteration += 1
        return loss.detach()

    @torch.no_grad()
    def validate(self, batches):
        """Eval-mode loss over the batches (pos_src/eval_utils.py:44-52): the mean of the per-batch ClassiferCriterion values.
        The model is left in the mode it was in."""
        was_training = self.model.training
        self.model.eval()
        total, n = 0.0, 0
        try:
            for b in batches:
                cap_r, new_mask = self._targets(b, b["feat_mask"].device)
                out = self.model(b["feat1"], b["feat2"], b["feat_mask"], None, None, cap_r, new_mask)
                cm = torch.as_tensor(b["class_mask"]).to(out.device)
                total += float(self.classify_crit(out, cap_r, b.get("cap_mask", new_mask), cm))
                n += 1
        finally:
            self.model.train(was_training)
        return total / max(n, 1)

    # ------------------------------------------------------------ checkpoints (starttrain_trainpos.py:200-238)
    def save_checkpoint(self, path, val_score=None, tag=""):
        os.makedirs(path, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(path, "model%s.pth" % tag))
        infos = dict(iter=self.iteration, epoch=self.epoch, best_val_score=self.best_val_score, opt=vars(self.opt),
                     val_score=val_score)
        torch.save(infos, os.path.join(path, "infos%s.pkl" % tag))

    def update_best(self, path, val_loss):
        """The best score is -val_loss; saves the best checkpoint and counts patience.  Returns True when training should stop."""
        score = -float(val_loss)
        if self.best_val_score is None or score > self.best_val_score:
            self.best_val_score = score
            self.patience = 0
            self.save_checkpoint(path, score, tag="-best")
            return False
        self.patience += 1
        return self.patience >= getattr(self.opt, "patience", 1 << 30)
