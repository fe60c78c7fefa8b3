#!/usr/bin/env python3
"""Timing of the POS sequence generator (docs/POS_GENERATOR.md).  Prints one JSON line:

  pos_step_us[BxK]      in-situ duration of one POS decoder step: device events around two greedy rollouts of the same batch
                        with seq_length 28 and 8, (t28 - t8) / 20 -- the encoder and the per-call prologue cancel
  captioner_step_us     the captioner's decoder-step launch group (xg_step_fwd, bench.measure_step_group) at the same B and K,
                        measured in the same process
  extract_ms            one extraction batch (extract_pos_features: teacher-forced forward + loss + greedy rollout, B 64, K 20)
  eager_ms              the same batch through tests/pos_oracle.py as eager PyTorch on the same GPU
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from controllable_xgating_amd import SAModel, make_opt  # noqa: E402
from controllable_xgating_amd.pos import PosModel, extract_pos_features  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tests.test_gpu_pos import make_opt as pos_opt  # noqa: E402


def pos_model(d):
    m = PosModel(pos_opt(d))
    P, run = po.make_params(d), po.make_running(d)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    return m.cuda().eval()


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def pos_step_us(B, K, reps):
    d = po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K))
    m = pos_model(d)
    x = po.make_inputs(d, seed=3)
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    t = {}
    for L in (28, 8):
        m.seq_length = L
        with torch.no_grad():
            t[L] = event_ms(lambda: m.sample(fr, fo, fm, {"sample_max": 1}), reps)
    m.seq_length = d.L
    return (t[28] - t[8]) / 20.0 * 1e3, t[28]


def captioner_step_us(B, K):
    cfg = dict(B=B, K=K, R=512, A=1536, E=468, V=20000, C=14, L=20, F1=1536, F2=1024)
    model = SAModel(make_opt(None, vocab_size=cfg["V"], seq_length=cfg["L"])).cuda()
    model.train()
    x = bench.synth_inputs(cfg["B"], cfg["K"], cfg["L"], cfg["V"], cfg["R"], cfg["F1"], cfg["F2"], cfg["C"], 0, "cuda")
    return bench.measure_step_group(model, x) * 1e6


def extraction_ms(reps):
    d = po.make_dims(**po.POS_CFG["full64"])
    m = pos_model(d)
    x = po.make_inputs(d, seed=4, ragged=True)
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap, cm = torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"])
    batch = [(fr, fo, fm, cap, cm, ["v%d" % i for i in range(d.B)])]
    with torch.no_grad():
        ours = wall_ms(lambda: extract_pos_features(m, batch, {}), reps)
    P = {k: v.cuda() for k, v in po.to_torch(po.make_params(d)).items()}
    run = {k: v.cuda() for k, v in po.to_torch(po.make_running(d)).items()}

    def eager():
        cap_r, new_mask = po.prepare_targets(cap, cm)
        cap_r, new_mask, cmd = cap_r.cuda(), new_mask.cuda(), cm.cuda()
        out = po.forward_tf(P, run, fr, fo, fm, cap_r, new_mask)
        float(po.criterion(out, cap_r, new_mask, cmd))
        states = po.sample_greedy(P, run, fr, fo, fm, d.L)[2]
        states.cpu()
    eager_t = wall_ms(eager, max(2, reps // 3))
    return ours, eager_t


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out = {"tool": "pos_bench", "gemm_mode": 0}
    for B, K in ((64, 20), (128, 26)):
        s, roll = pos_step_us(B, K, reps)
        out["pos_step_us[%dx%d]" % (B, K)] = round(s, 2)
        out["pos_rollout_ms[%dx%d]" % (B, K)] = round(roll, 3)
        out["captioner_step_us[%dx%d]" % (B, K)] = round(captioner_step_us(B, K), 2)
    ours, eager = extraction_ms(reps)
    out["extract_ms[64x20]"] = round(ours, 3)
    out["eager_ms[64x20]"] = round(eager, 3)
    out["speedup_vs_eager"] = round(eager / ours, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
