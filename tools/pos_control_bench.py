#!/usr/bin/env python3
"""Timing of controlled POS generation (docs/POS_GENERATOR.md, "Controlled generation").  One process; every GPU step runs under a
time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON
line and writes it to profiles/pos_control_bench.json (--out):

  forced_ms[S]          PosModel.sample_forced at B 64 videos, K 20, seq_length 28, S templates per video (device events, the best
                        of `reps` calls; trim=False: the call does not synchronise)
  forced_step_us[S]     in-situ duration of one decoder step over the 64 S rows: (t(L=28) - t(L=8)) / 20, as tools/pos_bench.py
  greedy_ms[S]          the only way to get 64 S rollouts without this entry point: PosModel.sample on the 64 videos repeated S
                        times (a batch of 64 S videos: encoder and operands replicated per row), same step count
  greedy_step_us[S]     its in-situ step
  forced_vs_greedy[S]   greedy_ms / forced_ms

  usage: pos_control_bench.py [reps] [--s 1,4,8] [--no-greedy] [--out PATH | --no-out]
"""
from __future__ import annotations

import contextlib
import faulthandler
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import pos_oracle as po  # noqa: E402
from tools.pos_bench import event_ms, pos_model  # noqa: E402

B, K, L_LONG, L_SHORT = 64, 20, 28, 8
STEP_LIMIT_S = 120


@contextlib.contextmanager
def step_limit(what, seconds=STEP_LIMIT_S):
    """A hard limit on one GPU step: the watchdog thread ends the process even when it waits inside the runtime."""
    print("[pos_control_bench] " + what, file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()


def forced_ms(m, feats, S, L, reps):
    g = torch.Generator().manual_seed(S)
    tm = torch.randint(1, m.category_size, (B, S, L), generator=g).cuda()       # no end tag: every step is live
    m.seq_length = L
    with torch.no_grad():
        return event_ms(lambda: m.sample_forced(*feats, tm, collect_states=True, trim=False), reps)


def greedy_ms(m, feats, S, L, reps):
    rep = [t.repeat_interleave(S, 0).contiguous() for t in feats]
    m.seq_length = L
    with torch.no_grad():
        return event_ms(lambda: m.sample(*rep, {"sample_max": 1}), reps)


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ss = [int(v) for v in argv[argv.index("--s") + 1].split(",")] if "--s" in argv else [1, 4, 8]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pos_control_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("pos_control_bench needs a GPU")
    d = po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K))
    with step_limit("model and inputs"):
        m = pos_model(d)
        x = po.make_inputs(d, seed=3)
        feats = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
    out = {"tool": "pos_control_bench", "B": B, "K": K, "seq_length": L_LONG, "reps": reps,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    for S in ss:
        t = {}
        for L in (L_LONG, L_SHORT):
            with step_limit("forced S=%d L=%d" % (S, L)):
                t[L] = forced_ms(m, feats, S, L, reps)
        out["forced_ms[%d]" % S] = round(t[L_LONG], 3)
        out["forced_step_us[%d]" % S] = round((t[L_LONG] - t[L_SHORT]) / (L_LONG - L_SHORT) * 1e3, 2)
        if "--no-greedy" in argv:
            continue
        g = {}
        for L in (L_LONG, L_SHORT):
            with step_limit("greedy on %d repeated videos L=%d" % (B * S, L)):
                g[L] = greedy_ms(m, feats, S, L, reps)
        out["greedy_ms[%d]" % S] = round(g[L_LONG], 3)
        out["greedy_step_us[%d]" % S] = round((g[L_LONG] - g[L_SHORT]) / (L_LONG - L_SHORT) * 1e3, 2)
        out["forced_vs_greedy[%d]" % S] = round(g[L_LONG] / t[L_LONG], 3)
    m.seq_length = d.L
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
