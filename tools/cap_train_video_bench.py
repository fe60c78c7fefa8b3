#!/usr/bin/env python3
"""Timing of teacher-forced training on Q captions per video (docs/CAPTION_TRAIN_PER_VIDEO.md).  One process; every GPU step runs
under a time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one
JSON line and writes it to profiles/cap_train_video_bench.json (--out).  BASELINE.json configs[1] layer sizes (K 26, R 512, A 1536,
V 20000, seq_length 20), 128 caption rows as B videos x Q captions, train mode, drop_prob_lm 0, no classifier term, captions of 20
words (every step is live), gradients accumulated into the bound flat buffer as the trainer has it.  `runs` (3) alternated runs of
the two ways to the same gradients, each the best of `reps` (10) calls of forward + backward WITHOUT the optimizer step, by device
events around the whole call:

  video_ms[BxQ]          SAModel.xe_loss_per_video + backward (include/xgate_train_video.h): the videos once
  repeat_ms[BxQ]         SAModel.xe_loss + backward on repeat_interleave'd inputs, the repeat inside the timed region.  The yardstick:
                         the parent's path, which this work leaves as it was
  *_spread[BxQ]          max - min over the runs
  ratio[BxQ]             mean repeat_ms / mean video_ms
  faster_every_run[BxQ]  video_ms < repeat_ms in every alternated run
  video_ws_bytes[BxQ]    xgtv_workspace_bytes;  repeat_ws_bytes[BxQ]: xg_workspace_bytes_mode(128-row dims, fp32)
  loss_diff[BxQ]         |loss difference| of the two
  max_grad_diff[BxQ]     the largest max |g_video - g_repeat| / max |g_repeat| over the parameters (those whose true gradient is zero
                         left out: tests/util.py ZERO_GRAD_PARAMS);  max_grad_diff_param[BxQ]: the parameter it belongs to

  usage: cap_train_video_bench.py [reps] [--shapes 32x4,16x8,128x1] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass [--only video|repeat]: no timing; two calls of each path (of the named one) at every shape, for a kernel trace taken
  around this process
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
    shapes = argv[argv.index("--shapes") + 1] if "--shapes" in argv else "32x4,16x8,128x1"
    shapes = [tuple(int(v) for v in s.split("x")) for s in shapes.split(",")]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    only = argv[argv.index("--only") + 1] if "--only" in argv else None
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_train_video_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_train_video_bench needs a GPU")
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_train_video as ntv
    d0 = pg.make_dims(**CFG["c1"])
    T = d0.L + 1
    with step_limit("model"):
        m = make_model(d0, train=True)
        m.flat_grads()                                            # gradients accumulate in place, as under train.ClipAdam

    def inputs(B, Q):
        d = d0._replace(B=B)
        x = pg.make_inputs(d, seed=3)
        r = pg.make_inputs(d0._replace(B=B * Q), seed=4)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        rows = [torch.from_numpy(r[k]).cuda() for k in ("pos_feats", "seq", "seq_mask")]
        return f, rows

    def video(f, rows, B, Q):
        loss = m.xe_loss_per_video(*f, rows[0].reshape(B, Q, -1), rows[1].reshape(B, Q, T), rows[2].reshape(B, Q, T))
        loss.backward()
        return loss

    def repeat(f, rows, B, Q):
        loss = m.xe_loss(f[0].repeat_interleave(Q, 0), f[1].repeat_interleave(Q, 0), f[2].repeat_interleave(Q, 0), *rows)
        loss.backward()
        return loss

    def grads_of(fn, *a):
        m._gflat.zero_()
        loss = fn(*a)
        torch.cuda.synchronize()
        return float(loss.item()), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    if "--profile-pass" in argv:
        for B, Q in shapes:
            f, rows = inputs(B, Q)
            with step_limit("profile pass %dx%d" % (B, Q)):
                for _ in range(2):
                    if only in (None, "video"):
                        video(f, rows, B, Q)
                    if only in (None, "repeat"):
                        repeat(f, rows, B, Q)
                torch.cuda.synchronize()
        return
    out = {"tool": "cap_train_video_bench", "K": d0.K, "R": d0.R, "A": d0.A, "V": d0.V, "seq_length": d0.L, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    for B, Q in shapes:
        key = "%dx%d" % (B, Q)
        f, rows = inputs(B, Q)
        with step_limit("gradients " + key):
            lv, gv = grads_of(video, f, rows, B, Q)
            lr, gr = grads_of(repeat, f, rows, B, Q)
            out["loss_diff[%s]" % key] = abs(lv - lr)
            worst = max((float((gv[n] - gr[n]).abs().max() / gr[n].abs().max().clamp_min(1e-30)), n)
                        for n in gv if n not in ZERO_GRAD_PARAMS)
            out["max_grad_diff[%s]" % key], out["max_grad_diff_param[%s]" % key] = worst
            del gv, gr
        dv, dr = m._dims(B, d0.K, T), m._dims(B * Q, d0.K, T)
        out["video_ws_bytes[%s]" % key] = int(ntv.lib().xgtv_workspace_bytes(C.byref(dv), Q))
        out["repeat_ws_bytes[%s]" % key] = int(nv.lib().xg_workspace_bytes_mode(C.byref(dr), 0))
        tv, tr = [], []
        for r in range(runs):                                     # alternated: video, repeat, video, repeat, ...
            with step_limit("run %d video %s" % (r, key)):
                tv.append(event_ms(lambda: video(f, rows, B, Q), reps))
            with step_limit("run %d repeat %s" % (r, key)):
                tr.append(event_ms(lambda: repeat(f, rows, B, Q), reps))
        out["video_ms[%s]" % key] = [round(v, 3) for v in tv]
        out["repeat_ms[%s]" % key] = [round(v, 3) for v in tr]
        out["video_ms_spread[%s]" % key] = round(max(tv) - min(tv), 3)
        out["repeat_ms_spread[%s]" % key] = round(max(tr) - min(tr), 3)
        out["ratio[%s]" % key] = round(mean(tr) / mean(tv), 3)
        out["faster_every_run[%s]" % key] = all(a_ < b_ for a_, b_ in zip(tv, tr))
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
