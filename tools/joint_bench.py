#!/usr/bin/env python3
"""Timing of joint training (docs/JOINT_TRAINING.md).  One process; every GPU step runs under a time limit of its own (a step that
overruns it ends the process with a traceback, and nothing more is started).  Reads nothing outside the repository.  Prints one JSON
line and writes it to profiles/joint_bench.json (--out).

Shapes: the captioner at BASELINE.json configs[1] layer sizes (K 26, R 512, A 1536, E 468, V 20000, C 14, seq_length 20) with 128
caption rows; the POS generator at its full-size layer sizes (R 512, A 1536, E 468, F1 1536, F2 1024) on the same batch -- 128 videos,
26 frames -- with the batch's own category count (14) and length (21 steps), since both models read the same cap_classes.  Train mode,
drop_prob_lm 0, weight_class 0.5, whole iterations: zero_grad, forward + loss, backward, clamp + Adam.  `runs` (3) alternated runs of
the lines, each the best of `reps` (10) iterations by device events around the whole iteration, every line warmed first:

  (a) xe_ms                 Trainer.train_batch, pos_feat a constant: the iteration as it was (the same launches as before)
  (b) xe_dpos_ms            the same with a pos_feat that requires a gradient: (a) + xgj_caption_dpos
      dpos_added_ms         mean xe_dpos_ms - mean xe_ms
  (c) pos_ms                PosTrainer.train_batch on the same batch
      separate_ms           xe_ms + pos_ms, run by run
      joint_ms              JointTrainer.train_batch (pos_loss_weight 0.5): (a) + (b)'s sum + the generator's iteration with
                            xgpj_final_state and the dpos input of its backward
      joint_minus_separate_ms   mean joint_ms - mean separate_ms
  *_spread                  max - min over the runs

  usage: joint_bench.py [reps] [--runs 3] [--rows 128] [--only-a] [--out PATH | --no-out]
  --only-a: line (a) alone, through nothing but Trainer -- the form that also runs on a tree without joint training, for the
            comparison with the commit before it
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import paramgen as pg  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tests.util import CFG, make_model  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 10
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    rows = int(argv[argv.index("--rows") + 1]) if "--rows" in argv else 128
    only_a = "--only-a" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "joint_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("joint_bench needs a GPU")
    from controllable_xgating_amd.driver import Trainer
    dc = pg.make_dims(**dict(CFG["c1"], B=rows))
    dp = po.make_dims(**dict(po.POS_CFG["full128"], B=rows, K=dc.K, C=dc.C, L=dc.L))
    assert (dp.R, dp.F1, dp.F2) == (dc.R, dc.F1, dc.F2)

    def opt(**kw):
        o = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, weight_class=0.5, learning_rate_decay_start=-1,
                               self_critical_after=-1, scheduled_sampling_start=-1, pos_loss_weight=0.5)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def pos_model():
        from controllable_xgating_amd.pos import PosModel
        m = PosModel(argparse.Namespace(category_size=dp.C, input_encoding_size=dp.E, rnn_size=dp.R, att_size=dp.A, num_layers=1,
                                        drop_prob_lm=0.0, seq_length=dp.L, feat_size=dp.F1, feat_size2=dp.F2))
        sd = po.make_state_dict(dp, po.make_params(dp), po.make_running(dp))
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        return m.cuda().train()

    xc, xp = pg.make_inputs(dc, seed=3, ragged=True), po.make_inputs(dp, seed=3, ragged=True)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    b = dict(feat1=t(xc["feats_rgb"]), feat2=t(xc["feats_opfl"]), feat_mask=t(xc["feat_mask"]), cap=t(xc["seq"]), cap_mask=t(xc["seq_mask"]),
             cap_classes=t(xp["cap_classes"]), class_mask=t(xp["class_mask"]), pos_feat=t(xc["pos_feats"]))
    with step_limit("models"):
        tr_a = Trainer(make_model(dc, train=True), opt())
        tr_a.start_epoch(0)
    lines = [("xe", lambda: tr_a.train_batch(b))]
    if not only_a:
        from controllable_xgating_amd import JointTrainer
        from controllable_xgating_amd.pos_train import PosTrainer
        with step_limit("models of the other lines"):
            tr_p = PosTrainer(pos_model(), opt())
            tr_p.start_epoch(0)
            tr_j = JointTrainer(make_model(dc, train=True), pos_model(), opt())
            tr_j.start_epoch(0)
        leaf = b["pos_feat"].clone().requires_grad_(True)
        b_leaf = dict(b, pos_feat=leaf)

        def xe_dpos():
            leaf.grad = None
            tr_a.train_batch(b_leaf)

        lines += [("xe_dpos", xe_dpos), ("pos", lambda: tr_p.train_batch(b)), ("joint", lambda: tr_j.train_batch(b))]
    out = {"tool": "joint_bench", "rows": rows, "K": dc.K, "R": dc.R, "A": dc.A, "V": dc.V, "seq_length": dc.L, "categories": dc.C,
           "reps": reps, "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    with step_limit("warm-up"):
        for _, fn in lines:
            for _ in range(3):
                fn()
    ms = {name: [] for name, _ in lines}
    for r in range(runs):                                         # alternated: xe, xe_dpos, pos, joint, xe, ...
        for name, fn in lines:
            with step_limit("run %d %s" % (r, name)):
                ms[name].append(event_ms(fn, reps))
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    if not only_a:
        ms["separate"] = [x + p for x, p in zip(ms["xe"], ms["pos"])]
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all())
    for name, v in ms.items():
        out["%s_ms" % name] = [round(x, 3) for x in v]
        out["%s_ms_spread" % name] = round(max(v) - min(v), 3)
    if not only_a:
        out["dpos_added_ms"] = round(mean(ms["xe_dpos"]) - mean(ms["xe"]), 4)
        out["joint_minus_separate_ms"] = round(mean(ms["joint"]) - mean(ms["separate"]), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
