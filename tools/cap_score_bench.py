#!/usr/bin/env python3
"""Timing of scoring given captions, Q caption rows per video (docs/CAPTION_SCORE.md).  One process; every GPU step runs under a time
limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line and
writes it to profiles/cap_score_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26, R 512, A 1536, V 20000,
seq_length 20), captions of 20 words without an end token (every step is live), Q rows per video, `runs` (3) alternated runs of the
two ways to the same log-probabilities, each the best of `reps` calls by device events around the WHOLE call (encoder included; both
return without a host synchronisation):

  score_ms[Q]           SAModel.score_captions_per_video (include/xgate_score.h): the videos once, no logits written
  replay_ms[Q]          SAModel.sample(..., {"forced_tokens": ..., "async": True}) on repeat_interleave'd inputs, the repeat inside the
                        timed region.  The yardstick: this work leaves it as it was
  *_spread[Q]           max - min over the runs
  ratio[Q]              mean replay_ms / mean score_ms
  faster_every_run[Q]   score_ms < replay_ms in every alternated run
  score_ws_bytes[Q]     xgsc_workspace_bytes;  replay_ws_bytes[Q]: the workspace sample() takes for the B*Q-row dims
  max_diff[Q]           max |tok_logp - seqLogprobs| over all rows and columns (every column is counted)

  usage: cap_score_bench.py [reps] [--q 1,8,64] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; two calls of each path at every Q, for a kernel trace taken around this process
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
    reps = int(argv[0]) if argv and argv[0].isdigit() else 10
    qs = [int(v) for v in argv[argv.index("--q") + 1].split(",")] if "--q" in argv else [1, 8, 64]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_score_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_score_bench needs a GPU")
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_score as nsc
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = {Q: torch.from_numpy(pg.uniform("pos_feats_q", (B * Q, d.R), 3, -1.0, 1.0)).cuda() for Q in qs}
        cap = {Q: torch.from_numpy(pg.randint("captions_q", (B * Q, d.L), 3, 1, d.V).astype("int64")).cuda() for Q in qs}

    def score(Q):
        return m.score_captions_per_video(*f, pos[Q].reshape(B, Q, d.R), cap[Q].reshape(B, Q, d.L))

    def replay(Q):
        return m.sample(f[0].repeat_interleave(Q, 0), f[1].repeat_interleave(Q, 0), f[2].repeat_interleave(Q, 0), pos[Q],
                        {"forced_tokens": cap[Q], "async": True})

    if "--profile-pass" in argv:
        with torch.no_grad():
            for Q in qs:
                with step_limit("profile pass Q=%d" % Q):
                    for _ in range(2):
                        score(Q)
                        replay(Q)
                    torch.cuda.synchronize()
        return
    out = {"tool": "cap_score_bench", "B": B, "K": d.K, "R": d.R, "A": d.A, "V": d.V, "seq_length": d.L, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        for Q in qs:
            with step_limit("log-probabilities Q=%d" % Q):
                a = score(Q)[0].reshape(B * Q, -1)
                b = replay(Q)[1]
                out["max_diff[%d]" % Q] = float((a - b).abs().max())
            dv, dr = m._dims(B, d.K, d.L + 1), m._dims(B * Q, d.K, d.L + 1)
            out["score_ws_bytes[%d]" % Q] = int(nsc.lib().xgsc_workspace_bytes(C.byref(dv), Q))
            out["replay_ws_bytes[%d]" % Q] = int(nv.lib().xg_workspace_bytes_mode(C.byref(dr), 0))
            ts, tr = [], []
            for r in range(runs):                                 # alternated: score, replay, score, replay, ...
                with step_limit("run %d score Q=%d" % (r, Q)):
                    ts.append(event_ms(lambda: score(Q), reps))
                with step_limit("run %d replay Q=%d" % (r, Q)):
                    tr.append(event_ms(lambda: replay(Q), reps))
            out["score_ms[%d]" % Q] = [round(v, 3) for v in ts]
            out["replay_ms[%d]" % Q] = [round(v, 3) for v in tr]
            out["score_ms_spread[%d]" % Q] = round(max(ts) - min(ts), 3)
            out["replay_ms_spread[%d]" % Q] = round(max(tr) - min(tr), 3)
            out["ratio[%d]" % Q] = round(mean(tr) / mean(ts), 3)
            out["faster_every_run[%d]" % Q] = all(a_ < b_ for a_, b_ in zip(ts, tr))
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
