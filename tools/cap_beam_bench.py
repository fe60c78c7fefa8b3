#!/usr/bin/env python3
"""Timing of the captioner's beam search (docs/CAPTION_BEAM.md).  One process; every GPU step runs under a time limit of its own (a
step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line and writes it to
profiles/cap_beam_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26, R 512, V 20000, seq_length 20), beam width
W, `runs` (3) alternated runs of the two ways to the same beams, each the best of `reps` (20) calls by device events around the
WHOLE call (encoder included):

  device_ms[W]          SAModel.beam_captions (include/xgate_beam.h): one enqueue, no host step
  host_ms[W]            SAModel.encode + beam.sample_beam: one xg_step_fwd group, a log-softmax, a top-k, a device-to-host copy and a
                        Python merge per step.  The yardstick: this work leaves it as it was
  *_spread[W]           max - min over the runs
  ratio[W]              mean host_ms / mean device_ms
  faster_every_run[W]   device_ms + both spreads < host_ms in every alternated run
  same_best[W]          share of videos whose best beam is the same caption on both paths (ties may differ within rounding)

  usage: cap_beam_bench.py [reps] [--w 1,5,8] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; three device calls and one host call at every W, for a kernel trace taken around this process
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import paramgen as pg  # noqa: E402
from tests.util import CFG, make_model  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402

B = 64


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ws = [int(v) for v in argv[argv.index("--w") + 1].split(",")] if "--w" in argv else [1, 5, 8]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_beam_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_beam_bench needs a GPU")
    from controllable_xgating_amd.beam import sample_beam
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats")]

    def device(W):
        return m.beam_captions(*f, beam_size=W)

    def host(W):
        return sample_beam(m, m.encode(*f[:3]), f[2], f[3], {"beam_size": W})

    if "--profile-pass" in argv:
        with torch.no_grad():
            for W in ws:
                with step_limit("profile pass W=%d" % W):
                    for _ in range(3):
                        device(W)
                    host(W)
        return
    out = {"tool": "cap_beam_bench", "B": B, "K": d.K, "R": d.R, "V": d.V, "seq_length": d.L, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        for W in ws:
            with step_limit("beams W=%d" % W):
                seq = device(W)[0][:, 0]
                hseq = host(W)[0].cuda()
                out["same_best[%d]" % W] = round(float((seq == hseq).all(1).float().mean()), 3)
            td, th = [], []
            for r in range(runs):                                 # alternated: device, host, device, host, ...
                with step_limit("run %d device W=%d" % (r, W)):
                    td.append(event_ms(lambda: device(W), reps))
                with step_limit("run %d host W=%d" % (r, W), 300):
                    th.append(event_ms(lambda: host(W), reps))
            sd, sh = max(td) - min(td), max(th) - min(th)
            out["device_ms[%d]" % W] = [round(v, 3) for v in td]
            out["host_ms[%d]" % W] = [round(v, 3) for v in th]
            out["device_ms_spread[%d]" % W] = round(sd, 3)
            out["host_ms_spread[%d]" % W] = round(sh, 3)
            out["ratio[%d]" % W] = round(mean(th) / mean(td), 2)
            out["faster_every_run[%d]" % W] = all(a + sd + sh < b for a, b in zip(td, th))
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
