#!/usr/bin/env python3
"""Timing of POS beam search (docs/POS_GENERATOR.md, "Beam templates").  One process; every GPU step runs under a time limit of
its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line and writes
it to profiles/pos_beam_bench.json (--out).  At B 64 videos, K 20, seq_length 28, beam width W, `runs` (3) alternated runs of the
two native calls, each the best of `reps` calls by device events (trim=False: neither call synchronises):

  beam_ms[W]            PosModel.beam_templates: one value per run
  beam_step_us[W]       in-situ duration of one search step over the 64 W rows: (t(L=28) - t(L=8)) / 20, as tools/pos_bench.py
  forced_ms[W]          PosModel.sample_forced at S = W on the very templates the search returned, without the states: the same
                        first three launches per step; its fourth launch has 64 W workgroups where the merge has 64
  forced_step_us[W]     its in-situ step
  *_spread[W]           max - min over the runs: the run-to-run spread the difference of the two is read against
  step_diff_us[W]       mean beam step - mean forced step: what the merge costs over the forced call's cell + head launch
  oracle_ms[W]          tests/pos_beam_oracle.beam_templates in float32 eager torch on the same GPU, one call (wall clock,
                        synchronised): the way to the same templates without this entry point

  usage: pos_beam_bench.py [reps] [--w 1,5,8] [--runs 3] [--out PATH | --no-out]
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import pos_beam_oracle as pbo  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tools.pos_bench import event_ms, pos_model  # noqa: E402
from tools.pos_control_bench import B, K, L_LONG, L_SHORT, step_limit  # noqa: E402


def beam_ms(m, feats, W, L, reps):
    m.seq_length = L
    with torch.no_grad():
        return event_ms(lambda: m.beam_templates(*feats, beam_size=W, trim=False), reps)


def forced_ms(m, feats, tm, reps):
    m.seq_length = tm.shape[2]
    with torch.no_grad():
        return event_ms(lambda: m.sample_forced(*feats, tm, collect_states=False, trim=False), reps)


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ws = [int(v) for v in argv[argv.index("--w") + 1].split(",")] if "--w" in argv else [1, 5, 8]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pos_beam_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("pos_beam_bench needs a GPU")
    d = po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K))
    with step_limit("model and inputs"):
        m = pos_model(d)
        x = po.make_inputs(d, seed=3)
        feats = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        Pt = {k: v.detach() for k, v in m.state_dict().items()}
    out = {"tool": "pos_beam_bench", "B": B, "K": K, "seq_length": L_LONG, "reps": reps, "runs": runs,
           "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)
    for W in ws:
        tm = {}
        with step_limit("templates W=%d" % W):
            for L in (L_LONG, L_SHORT):
                m.seq_length = L
                with torch.no_grad():
                    tm[L] = m.beam_templates(*feats, beam_size=W, trim=False)[0]
            live = float((tm[L_LONG] > 0).float().mean())
        tb, tf = {L: [] for L in tm}, {L: [] for L in tm}
        for r in range(runs):                                    # alternated: beam, forced, beam, forced, ...
            for L in (L_LONG, L_SHORT):
                with step_limit("run %d beam W=%d L=%d" % (r, W, L)):
                    tb[L].append(beam_ms(m, feats, W, L, reps))
                with step_limit("run %d forced W=%d L=%d" % (r, W, L)):
                    tf[L].append(forced_ms(m, feats, tm[L], reps))
        with step_limit("oracle W=%d" % W):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = pbo.beam_templates(Pt, Pt, *feats, L_LONG, W)
            torch.cuda.synchronize()
            out["oracle_ms[%d]" % W] = round((time.perf_counter() - t0) * 1e3, 1)
            out["oracle_same_templates[%d]" % W] = round(float((torch.from_numpy(o["templates"]).cuda() == tm[L_LONG]).all(2).float().mean()), 3)
        step = lambda t: [(a - b) / (L_LONG - L_SHORT) * 1e3 for a, b in zip(t[L_LONG], t[L_SHORT])]
        bs_us, fs_us = step(tb), step(tf)
        out["live_tag_share[%d]" % W] = round(live, 3)
        out["beam_ms[%d]" % W] = [round(v, 3) for v in tb[L_LONG]]
        out["forced_ms[%d]" % W] = [round(v, 3) for v in tf[L_LONG]]
        out["beam_step_us[%d]" % W] = [round(v, 2) for v in bs_us]
        out["forced_step_us[%d]" % W] = [round(v, 2) for v in fs_us]
        out["beam_ms_spread[%d]" % W] = round(max(tb[L_LONG]) - min(tb[L_LONG]), 3)
        out["forced_ms_spread[%d]" % W] = round(max(tf[L_LONG]) - min(tf[L_LONG]), 3)
        out["beam_step_spread_us[%d]" % W] = round(max(bs_us) - min(bs_us), 2)
        out["forced_step_spread_us[%d]" % W] = round(max(fs_us) - min(fs_us), 2)
        out["step_diff_us[%d]" % W] = round(mean(bs_us) - mean(fs_us), 2)
    m.seq_length = d.L
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
