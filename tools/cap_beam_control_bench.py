#!/usr/bin/env python3
"""Timing of the captioner's beam search under S POS vectors per video (docs/CAPTION_BEAM_CONTROL.md).  One process; every GPU step
runs under a time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints
one JSON line and writes it to profiles/cap_beam_control_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26,
R 512, A 1536, V 20000, seq_length 20), beam width W (5), S rows per video, `runs` (3) alternated runs of the two ways to the same
beams, each the best of `reps` (20) calls by device events around the WHOLE call (encoder included; both return without a host
synchronisation):

  shared_ms[S]          SAModel.beam_captions_per_video (include/xgate_beam_control.h): the videos once, V and v2a(V) not repeated,
                        the group attention, the threshold selection
  repeated_ms[S]        SAModel.beam_captions on repeat_interleave'd inputs, the repeat inside the timed region.  The yardstick: this
                        work leaves it as it was
  *_spread[S]           max - min over the runs
  ratio[S]              mean repeated_ms / mean shared_ms
  faster_every_run[S]   shared_ms < repeated_ms in every alternated run
  shared_ws_bytes[S]    xgbc_workspace_bytes;  repeated_ws_bytes[S]: xgcb_workspace_bytes at B*S videos
  same_best[S]          (video, template) pairs whose best beam is the same caption on both paths, of B*S (ties may differ within
                        rounding)

  usage: cap_beam_control_bench.py [reps] [--s 1,4,8] [--w 5] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; three calls of each path at every S, for a kernel trace taken around this process
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
from tests.util import CFG, make_model  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402

B = 64


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ss = [int(v) for v in argv[argv.index("--s") + 1].split(",")] if "--s" in argv else [1, 4, 8]
    W = int(argv[argv.index("--w") + 1]) if "--w" in argv else 5
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_beam_control_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_beam_control_bench needs a GPU")
    from controllable_xgating_amd import _native_beam as nb
    from controllable_xgating_amd import _native_beam_control as nbc
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = {S: torch.from_numpy(pg.uniform("pos_feats_s", (B * S, d.R), 3, -1.0, 1.0)).cuda() for S in ss}

    def shared(S):
        return m.beam_captions_per_video(*f, pos[S].reshape(B, S, d.R), beam_size=W)

    def repeated(S):
        return m.beam_captions(f[0].repeat_interleave(S, 0), f[1].repeat_interleave(S, 0), f[2].repeat_interleave(S, 0), pos[S],
                               beam_size=W)

    if "--profile-pass" in argv:
        with torch.no_grad():
            for S in ss:
                with step_limit("profile pass S=%d" % S):
                    for _ in range(3):
                        shared(S)
                        repeated(S)
                    torch.cuda.synchronize()
        return
    out = {"tool": "cap_beam_control_bench", "B": B, "W": W, "K": d.K, "R": d.R, "A": d.A, "V": d.V, "seq_length": d.L, "reps": reps,
           "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        for S in ss:
            with step_limit("beams S=%d" % S):
                a = shared(S)[0].reshape(B * S, W, -1)[:, 0]
                b = repeated(S)[0][:, 0]
                out["same_best[%d]" % S] = "%d of %d" % (int((a == b).all(1).sum()), B * S)
            dv, dr = m._dims(B, d.K, d.L + 1), m._dims(B * S, d.K, d.L + 1)
            out["shared_ws_bytes[%d]" % S] = int(nbc.lib().xgbc_workspace_bytes(C.byref(dv), S, W))
            out["repeated_ws_bytes[%d]" % S] = int(nb.lib().xgcb_workspace_bytes(C.byref(dr), W))
            ts, tr = [], []
            for r in range(runs):                                 # alternated: shared, repeated, shared, repeated, ...
                with step_limit("run %d shared S=%d" % (r, S)):
                    ts.append(event_ms(lambda: shared(S), reps))
                with step_limit("run %d repeated S=%d" % (r, S)):
                    tr.append(event_ms(lambda: repeated(S), reps))
            out["shared_ms[%d]" % S] = [round(v, 3) for v in ts]
            out["repeated_ms[%d]" % S] = [round(v, 3) for v in tr]
            out["shared_ms_spread[%d]" % S] = round(max(ts) - min(ts), 3)
            out["repeated_ms_spread[%d]" % S] = round(max(tr) - min(tr), 3)
            out["ratio[%d]" % S] = round(mean(tr) / mean(ts), 3)
            out["faster_every_run[%d]" % S] = all(a_ < b_ for a_, b_ in zip(ts, tr))
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
