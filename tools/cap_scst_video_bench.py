#!/usr/bin/env python3
"""Timing of self-critical training on S rollouts per video (docs/CAPTION_SCST_PER_VIDEO.md).  One process; every GPU step runs under
a time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON
line and writes it to profiles/cap_scst_video_bench.json (--out).  BASELINE.json configs[2] layer sizes (K 26, R 512, A 1536, V 20000),
seq_length 30, B videos x S rollouts, train mode, drop_prob_lm 0, fixed uniforms and scores, gradients accumulated into the bound flat
buffer as the trainer has it.  `runs` (3) alternated runs of the two ways to the same gradients, each the best of `reps` (10) calls of
rollout + criterion + backward WITHOUT the optimizer step, by device events around the whole call:

  video_ms[BxS]          SAModel.rollout_per_video + PerVideoRewardCriterion + backward (include/xgate_scst_video.h): the videos once
                         ("mean_others"; S = 1: a given base per video)
  repeat_ms[BxS]         SAModel.sample(sample_max 0) with gradients on repeat_interleave'd inputs (the repeat inside the timed
                         region) + RewardCriterion on the same advantages + backward.  The yardstick: the parent's path
  *_spread[BxS]          max - min over the runs
  ratio[BxS]             mean repeat_ms / mean video_ms
  faster_every_run[BxS]  video_ms < repeat_ms in every alternated run
  video_ws_bytes[BxS]    xgsv_workspace_bytes;  repeat_ws_bytes[BxS]: xg_workspace_bytes_mode(B S-row dims, fp32)
  width[BxS]             the rollouts' early-exit width
  rows_differ[BxS]       rows in which the two paths DREW different tokens from the same uniforms (a draw whose uniform lies at an
                         edge of the CDF may take either neighbour: the two paths' logits differ in their last bits)
  loss_diff[BxS], max_grad_diff[BxS], max_grad_diff_param[BxS]   as tools/cap_train_video_bench.py has them, with the repeated batch
                         REPLAYING the per-video call's tokens (forced_tokens), so that both differentiate the same captions;
  replay_logp_diff[BxS]  the largest |seqLogprobs difference| of that replay over the counted words, the rows that differ among them
  pair_ms, pair_ms_spread   the reference-shaped iteration at B = 64: SAModel.sample_pair (sampled + greedy rollout) + RewardCriterion +
                         backward, alternated with video_ms[64x5] (pair_vs_64x5: mean video_ms[64x5] / mean pair_ms)

  usage: cap_scst_video_bench.py [reps] [--shapes 32x4,16x8,64x5,128x1] [--runs 3] [--out PATH | --no-out]
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import paramgen as pg  # noqa: E402
from tests.util import CFG, ZERO_GRAD_PARAMS, make_model  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 10
    shapes = argv[argv.index("--shapes") + 1] if "--shapes" in argv else "32x4,16x8,64x5,128x1"
    shapes = [tuple(int(v) for v in s.split("x")) for s in shapes.split(",")]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_scst_video_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_scst_video_bench needs a GPU")
    from controllable_xgating_amd import PerVideoRewardCriterion, RewardCriterion
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_scst_video as nsv
    d0 = pg.make_dims(**dict(CFG["c1"], L=30))
    T = d0.L + 1
    with step_limit("model"):
        m = make_model(d0, train=True)
        m.flat_grads()                                            # gradients accumulate in place, as under train.ClipAdam
    crit_v, crit_r = PerVideoRewardCriterion(), RewardCriterion()

    def inputs(B, S):
        x = pg.make_inputs(d0._replace(B=B), seed=3)
        r = pg.make_inputs(d0._replace(B=B * S), seed=4)
        g = torch.Generator().manual_seed(B * 1000 + S)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = torch.from_numpy(r["pos_feats"]).cuda()
        u = torch.rand(T, B * S, generator=g).cuda()
        score, base = torch.rand(B, S, generator=g).cuda(), torch.rand(B, generator=g).cuda()
        adv = (score - (score.sum(1, keepdim=True) - score) / (S - 1)) if S > 1 else score - base[:, None]
        return f, pos, u, score, base, adv.reshape(B * S, 1).contiguous()

    def video(f, pos, u, score, base, adv, B, S):
        seq, slp, n = m.rollout_per_video(*f, pos.reshape(B, S, -1), uniforms=u)
        loss = crit_v(slp, seq, score, n=n, baseline="mean_others" if S > 1 else base)
        loss.backward()
        return loss, seq.reshape(B * S, -1), n

    def repeat_fwd(f, pos, u, score, base, adv, B, S):
        seq, _, n = m.sample(f[0].repeat_interleave(S, 0), f[1].repeat_interleave(S, 0), f[2].repeat_interleave(S, 0), pos,
                             {"sample_max": 0, "uniforms": u, "async": True})
        return seq, n

    def repeat(f, pos, u, score, base, adv, B, S):
        seq, slp, n = m.sample(f[0].repeat_interleave(S, 0), f[1].repeat_interleave(S, 0), f[2].repeat_interleave(S, 0), pos,
                               {"sample_max": 0, "uniforms": u, "async": True})
        loss = crit_r(slp, seq, adv, n=n)
        loss.backward()
        return loss, seq, n

    def replay(f, pos, u, score, base, adv, B, S, tokens):
        seq, slp = m.sample(f[0].repeat_interleave(S, 0), f[1].repeat_interleave(S, 0), f[2].repeat_interleave(S, 0), pos,
                            {"sample_max": 0, "forced_tokens": tokens})
        loss = crit_r(slp, seq, adv)
        loss.backward()
        return loss, slp.detach()

    def pair(f, pos, u, adv):
        gen, slp, greedy, n = m.sample_pair(*f, pos, {"sample_max": 0, "uniforms": u, "async": True})
        loss = crit_r(slp, gen, adv, n=n[:1])
        loss.backward()
        return loss

    def grads_of(fn, *a):
        m._gflat.zero_()
        res = fn(*a)
        torch.cuda.synchronize()
        return (float(res[0].item()),) + tuple(res[1:]) + ({k: p.grad.detach().clone() for k, p in m.named_parameters()},)

    out = {"tool": "cap_scst_video_bench", "K": d0.K, "R": d0.R, "A": d0.A, "V": d0.V, "seq_length": d0.L, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    for B, S in shapes:
        key = "%dx%d" % (B, S)
        a = inputs(B, S) + (B, S)
        with step_limit("gradients " + key):
            lv, sv, nv_, gv = grads_of(video, *a)
            sv, nv_ = sv.clone(), int(nv_.item())
            with torch.no_grad():
                sr, nr = repeat_fwd(*a)
            out["width[%s]" % key] = nv_
            out["rows_differ[%s]" % key] = int((sv != sr).any(1).sum().item()) if int(nr.item()) == nv_ else -1
            with torch.no_grad():
                slp_v = m.rollout_per_video(*a[0], a[1].reshape(B, S, -1), uniforms=a[2])[1].reshape(B * S, -1)[:, :nv_]
            lr, slp_r, gr = grads_of(replay, *a, sv[:, :nv_].contiguous())
            mask = torch.cat([torch.ones_like(sv[:, :1], dtype=torch.bool), sv[:, :nv_ - 1] > 0], 1)
            out["replay_logp_diff[%s]" % key] = float((slp_v - slp_r)[mask].abs().max().item())
            out["loss_diff[%s]" % key] = abs(lv - lr)
            worst = max((float((gv[k] - gr[k]).abs().max() / gr[k].abs().max().clamp_min(1e-30)), k)
                        for k in gv if k not in ZERO_GRAD_PARAMS)
            out["max_grad_diff[%s]" % key], out["max_grad_diff_param[%s]" % key] = worst
            del gv, gr
        dv, dr = m._dims(B, d0.K, T), m._dims(B * S, d0.K, T)
        out["video_ws_bytes[%s]" % key] = int(nsv.lib().xgsv_workspace_bytes(C.byref(dv), S))
        out["repeat_ws_bytes[%s]" % key] = int(nv.lib().xg_workspace_bytes_mode(C.byref(dr), 0))
        tv, tr, tp = [], [], []
        with_pair = (B, S) == (64, 5)
        if with_pair:
            fp, posp, up, _, _, advp = inputs(64, 1)
        for r in range(runs):                                     # alternated: video, repeat (, pair), video, repeat, ...
            with step_limit("run %d video %s" % (r, key)):
                tv.append(event_ms(lambda: video(*a), reps))
            with step_limit("run %d repeat %s" % (r, key)):
                tr.append(event_ms(lambda: repeat(*a), reps))
            if with_pair:
                with step_limit("run %d pair" % r):
                    tp.append(event_ms(lambda: pair(fp, posp, up, advp), reps))
        out["video_ms[%s]" % key] = [round(v, 3) for v in tv]
        out["repeat_ms[%s]" % key] = [round(v, 3) for v in tr]
        out["video_ms_spread[%s]" % key] = round(max(tv) - min(tv), 3)
        out["repeat_ms_spread[%s]" % key] = round(max(tr) - min(tr), 3)
        out["ratio[%s]" % key] = round(mean(tr) / mean(tv), 3)
        out["faster_every_run[%s]" % key] = all(a_ < b_ for a_, b_ in zip(tv, tr))
        if with_pair:
            out["pair_ms"] = [round(v, 3) for v in tp]
            out["pair_ms_spread"] = round(max(tp) - min(tp), 3)
            out["pair_vs_64x5"] = round(mean(tv) / mean(tp), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
