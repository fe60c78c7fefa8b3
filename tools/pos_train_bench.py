#!/usr/bin/env python3
"""Timing of one POS generator training iteration (docs/POS_GENERATOR.md, "Training").  Prints one JSON line and writes it to
profiles/pos_train_bench.json (or the path given as the first argument):

  iter_ms[BxK]          zero_grad + train-mode forward + ClassiferCriterion + backward + clamp + Adam (PosTrainer.train_batch),
                        device events around `iters` iterations after warm-up, seq_length 28, p = 0.5 (run_train.sh)
  eager_ms[BxK]         the same iteration as eager PyTorch autograd of tests/pos_train_oracle.py + torch.optim.Adam + clamp on the
                        same GPU, with the dropout masks built once before the timed loop and kept on the device (the host-side
                        hash is not part of it); like the reference it reads each step's category column sum on the host
  speedup[BxK]          eager_ms / iter_ms
  bwd_fwd_step_us       in-situ cost of one decoder step, forward + backward: (t(L 28) - t(L 14)) / 14 at B 64, K 20 (the encoder,
                        its backward and the update cancel)
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

from controllable_xgating_amd.pos import PosModel, prepare_pos_targets  # noqa: E402
from controllable_xgating_amd.pos_train import PosTrainer  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tests import pos_train_oracle as pto  # noqa: E402


def dims(B, K, L):
    return po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K, L=L))


def setup(d, p):
    P, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, seed=0, ragged=True)
    opt = argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1, drop_prob_lm=p,
                             seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)
    m = PosModel(opt)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    m = m.cuda().train()
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    b = dict(feat1=fr, feat2=fo, feat_mask=fm, cap_classes=torch.from_numpy(x["cap_classes"]).cuda(),
             class_mask=torch.from_numpy(x["class_mask"]).cuda())
    return P, run, x, m, b


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def hip_iter_ms(d, p, warmup, iters):
    _, _, _, m, b = setup(d, p)
    tr = PosTrainer(m, argparse.Namespace(learning_rate=4e-4, grad_clip=0.1, learning_rate_decay_start=-1))
    tr.start_epoch(0)
    return timed(lambda: tr.train_batch(b), warmup, iters)


def eager_iter_ms(d, p, warmup, iters):
    P, run, x, _, _ = setup(d, p)
    Pt, rt = pto.params(P, device="cuda"), pto.running(run, device="cuda")
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = prepare_pos_targets(torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"]))
    cap_r, new_mask, cm = cap_r.cuda(), new_mask.cuda(), torch.from_numpy(x["class_mask"]).cuda()
    opt = torch.optim.Adam(list(Pt.values()), lr=4e-4)
    masks = {}            # the hash masks, built on the host once (in the warm-up) and kept on the device: not timed

    def it():
        opt.zero_grad()
        out = pto.forward_train(Pt, rt, fr, fo, fm, cap_r, new_mask, p, 1, cache=masks)
        loss = pto.criterion(out, cap_r, new_mask, cm)
        loss.backward()
        for v in Pt.values():
            v.grad.data.clamp_(-0.1, 0.1)
        opt.step()
    assert warmup >= 1
    return timed(it, warmup, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pos_train_bench.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eager-iters", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    p = 0.5
    res = {"p": p, "L": 28, "eager_masks": "prebuilt on the device, outside the timed loop"}
    for B, K in ((64, 20), (128, 26)):
        d = dims(B, K, 28)
        key = "%dx%d" % (B, K)
        res["iter_ms[%s]" % key] = round(hip_iter_ms(d, p, a.warmup, a.iters), 3)
        res["eager_ms[%s]" % key] = round(eager_iter_ms(d, p, 1, a.eager_iters), 3)
        res["speedup[%s]" % key] = round(res["eager_ms[%s]" % key] / res["iter_ms[%s]" % key], 2)
    t28 = res["iter_ms[64x20]"]
    t14 = hip_iter_ms(dims(64, 20, 14), p, a.warmup, a.iters)
    res["iter_ms[64x20,L14]"] = round(t14, 3)
    res["bwd_fwd_step_us"] = round((t28 - t14) / 14 * 1000.0, 1)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
