#!/usr/bin/env python3
"""Timing of diverse POS beam search (docs/POS_GENERATOR.md, "Diverse templates"), on the inputs of tools/pos_beam_bench.py.  One
process; every GPU step runs under a time limit of its own (a step that overruns it ends the process with a traceback, and nothing
more is started).  Prints one JSON line and writes it to profiles/pos_beam_diverse_bench.json (--out).  At B 64 videos, K 20,
seq_length 28, Gd groups of Wg slots (N = Gd Wg), `runs` (3) alternated runs of the two native calls, each the best of `reps` (20)
calls by device events around the whole call (trim=False: neither call synchronises):

  diverse_ms            PosModel.beam_templates_diverse (include/xgate_pos_beam_diverse.h) at lambda 0.5
  plain_ms              PosModel.beam_templates at W = N on the same inputs: untouched by this work, the yardstick
  *_spread              max - min over the runs
  ratio                 mean diverse_ms / mean plain_ms
  templates[lambda]     distinct templates per video among its N (control.first_occurrences), mean over the videos, for lambda 0.2,
                        0.5, 1 and for the plain search ("plain")
  first_tags[lambda]    distinct first tags among a video's N templates, likewise

  usage: pos_beam_diverse_bench.py [reps] [--groups 2] [--group-size 4] [--runs 3] [--out PATH | --no-out]
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from controllable_xgating_amd import first_occurrences  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tools.pos_bench import event_ms, pos_model  # noqa: E402
from tools.pos_control_bench import B, K, step_limit  # noqa: E402

LAMBDAS = (0.2, 0.5, 1.0)


def distinct(tm):
    """(B, N, L) templates -> (mean distinct templates, mean distinct first tags) per video."""
    n = first_occurrences(tm).sum(1).float().mean().item()
    t = tm[:, :, 0].cpu()
    return round(n, 3), round(sum(len(set(r.tolist())) for r in t) / t.shape[0], 3)


def main():
    argv = sys.argv[1:]
    arg = lambda k, dflt: int(argv[argv.index(k) + 1]) if k in argv else dflt      # noqa: E731
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    Gd, Wg, runs = arg("--groups", 2), arg("--group-size", 4), arg("--runs", 3)
    N = Gd * Wg
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "pos_beam_diverse_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("pos_beam_diverse_bench needs a GPU")
    d = po.make_dims(**dict(po.POS_CFG["full64"], B=B, K=K))
    with step_limit("model and inputs"):
        m = pos_model(d)
        x = po.make_inputs(d, seed=3)
        feats = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]

    def diverse(lam=0.5):
        return m.beam_templates_diverse(*feats, Gd, Wg, diversity=lam, trim=False)

    def plain():
        return m.beam_templates(*feats, beam_size=N, trim=False)

    out = {"tool": "pos_beam_diverse_bench", "B": B, "K": K, "groups": Gd, "group_size": Wg, "seq_length": d.L, "reps": reps,
           "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        with step_limit("diversity"):
            tp, ft = {}, {}
            for lam in LAMBDAS:
                tp[str(lam)], ft[str(lam)] = distinct(diverse(lam)[0].flatten(1, 2))
            tp["plain"], ft["plain"] = distinct(plain()[0])
            out["templates"], out["first_tags"] = tp, ft
        td, tpl = [], []
        for r in range(runs):                                     # alternated: diverse, plain, diverse, plain, ...
            with step_limit("run %d diverse" % r):
                td.append(event_ms(diverse, reps))
            with step_limit("run %d plain" % r):
                tpl.append(event_ms(plain, reps))
    out["diverse_ms"] = [round(v, 3) for v in td]
    out["plain_ms"] = [round(v, 3) for v in tpl]
    out["diverse_ms_spread"] = round(max(td) - min(td), 3)
    out["plain_ms_spread"] = round(max(tpl) - min(tpl), 3)
    out["ratio"] = round(mean(td) / mean(tpl), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
