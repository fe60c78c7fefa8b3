#!/usr/bin/env python3
"""Timing of sampled POS templates (docs/POS_GENERATOR.md, "Sampled templates").  One process; every GPU step runs under a time
limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line
and writes it to profiles/pos_sample_bench.json (--out).  At B 64 videos, K 20, seq_length 28, S rollouts per video, `runs`
(3) alternated runs of the two calls, each the best of `reps` calls by device events (trim=False: neither call synchronises):

  sampled_ms[S]         PosModel.sample_templates, uniforms already on the device: one value per run
  sampled_step_us[S]    in-situ duration of one decoder step over the 64 S rows: (t(L=28) - t(L=8)) / 20, as tools/pos_bench.py
  forced_ms[S]          PosModel.sample_forced on the very templates the sampled call produced: the fastest way to the same
                        states without this entry point (the two calls differ only in the step's last launch)
  forced_step_us[S]     its in-situ step
  *_spread[S]           max - min over the runs: the run-to-run spread the difference of the two is read against
  step_diff_us[S]       mean sampled step - mean forced step

  usage: pos_sample_bench.py [reps] [--s 1,4,8] [--runs 3] [--out PATH | --no-out]
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import pos_oracle as po  # noqa: E402
from tools.pos_bench import event_ms, pos_model  # noqa: E402
from tools.pos_control_bench import B, K, L_LONG, L_SHORT, step_limit  # noqa: E402


def sampled_ms(m, feats, u, S, reps):
    m.seq_length = u.shape[2]
    with torch.no_grad():
        return event_ms(lambda: m.sample_templates(*feats, S, uniforms=u, collect_states=True, trim=False), reps)


def forced_ms(m, feats, tm, reps):
    m.seq_length = tm.shape[2]
    with torch.no_grad():
        return event_ms(lambda: m.sample_forced(*feats, tm, collect_states=True, trim=False), reps)


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ss = [int(v) for v in argv[argv.index("--s") + 1].split(",")] if "--s" in argv else [1, 4, 8]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pos_sample_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("pos_sample_bench needs a GPU")
    d = po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K))
    with step_limit("model and inputs"):
        m = pos_model(d)
        x = po.make_inputs(d, seed=3)
        feats = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
    out = {"tool": "pos_sample_bench", "B": B, "K": K, "seq_length": L_LONG, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)
    for S in ss:
        g = torch.Generator(device="cuda").manual_seed(S)
        u, tm = {}, {}
        with step_limit("templates S=%d" % S):
            for L in (L_LONG, L_SHORT):
                u[L] = torch.rand(B, S, L, device="cuda", generator=g)
                m.seq_length = L
                with torch.no_grad():
                    tm[L] = m.sample_templates(*feats, S, uniforms=u[L], trim=False)[0]
            live = float((tm[L_LONG] > 0).float().mean())
        ts, tf = {L: [] for L in u}, {L: [] for L in u}
        for r in range(runs):                                    # alternated: sampled, forced, sampled, forced, ...
            for L in (L_LONG, L_SHORT):
                with step_limit("run %d sampled S=%d L=%d" % (r, S, L)):
                    ts[L].append(sampled_ms(m, feats, u[L], S, reps))
                with step_limit("run %d forced S=%d L=%d" % (r, S, L)):
                    tf[L].append(forced_ms(m, feats, tm[L], reps))
        step = lambda t: [(a - b) / (L_LONG - L_SHORT) * 1e3 for a, b in zip(t[L_LONG], t[L_SHORT])]
        ss_us, fs_us = step(ts), step(tf)
        out["live_tag_share[%d]" % S] = round(live, 3)
        out["sampled_ms[%d]" % S] = [round(v, 3) for v in ts[L_LONG]]
        out["forced_ms[%d]" % S] = [round(v, 3) for v in tf[L_LONG]]
        out["sampled_step_us[%d]" % S] = [round(v, 2) for v in ss_us]
        out["forced_step_us[%d]" % S] = [round(v, 2) for v in fs_us]
        out["sampled_ms_spread[%d]" % S] = round(max(ts[L_LONG]) - min(ts[L_LONG]), 3)
        out["forced_ms_spread[%d]" % S] = round(max(tf[L_LONG]) - min(tf[L_LONG]), 3)
        out["sampled_step_spread_us[%d]" % S] = round(max(ss_us) - min(ss_us), 2)
        out["forced_step_spread_us[%d]" % S] = round(max(fs_us) - min(fs_us), 2)
        out["step_diff_us[%d]" % S] = round(mean(ss_us) - mean(fs_us), 2)
    m.seq_length = d.L
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
