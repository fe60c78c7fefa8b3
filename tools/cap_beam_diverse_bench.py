#!/usr/bin/env python3
"""Timing of the captioner's diverse beam search (docs/CAPTION_DIVERSE.md), on the inputs of tools/cap_beam_control_bench.py.  One
process; every GPU step runs under a time limit of its own (a step that overruns it ends the process with a traceback, and nothing
more is started).  Prints one JSON line and writes it to profiles/cap_beam_diverse_bench.json (--out).  At B 64 videos of
BASELINE.json configs[1] (K 26, R 512, A 1536, V 20000, seq_length 20), S rows per video, Gd groups of Wg slots (N = Gd Wg), `runs`
(3) alternated runs, each the best of `reps` (20) calls by device events around the WHOLE call (encoder included; neither call
synchronises with the host):

  diverse_ms            SAModel.beam_captions_diverse (include/xgate_beam_diverse.h) at lambda 0.5
  plain_ms              SAModel.beam_captions_per_video at W = N on the same inputs: untouched by this work, the yardstick
  *_spread              max - min over the runs
  ratio                 mean diverse_ms / mean plain_ms
  first_words[lambda]   distinct first words among a pair's N captions, mean over the B S pairs, for lambda 0.2, 0.5, 1 and for
                        the plain search ("plain")
  captions[lambda]      distinct captions among a pair's N captions, likewise

  usage: cap_beam_diverse_bench.py [reps] [--s 4] [--groups 2] [--group-size 4] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; three calls of each path, for a kernel trace taken around this process
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
LAMBDAS = (0.2, 0.5, 1.0)


def distinct(seq):
    """(pairs, N, L) tokens -> (mean distinct first words, mean distinct captions) per pair."""
    s = seq.cpu()
    first = sum(len(set(r[:, 0].tolist())) for r in s) / s.shape[0]
    caps = sum(len({tuple(c.tolist()) for c in r}) for r in s) / s.shape[0]
    return round(first, 3), round(caps, 3)


def main():
    argv = sys.argv[1:]
    arg = lambda k, dflt: int(argv[argv.index(k) + 1]) if k in argv else dflt      # noqa: E731
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    S, Gd, Wg, runs = arg("--s", 4), arg("--groups", 2), arg("--group-size", 4), arg("--runs", 3)
    N = Gd * Wg
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_beam_diverse_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_beam_diverse_bench needs a GPU")
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = torch.from_numpy(pg.uniform("pos_feats_s", (B * S, d.R), 3, -1.0, 1.0)).cuda().reshape(B, S, d.R)

    def diverse(lam=0.5):
        return m.beam_captions_diverse(*f, pos, Gd, Wg, diversity=lam)

    def plain():
        return m.beam_captions_per_video(*f, pos, beam_size=N)

    if "--profile-pass" in argv:
        with torch.no_grad(), step_limit("profile pass"):
            for _ in range(3):
                diverse()
                plain()
            torch.cuda.synchronize()
        return
    out = {"tool": "cap_beam_diverse_bench", "B": B, "S": S, "groups": Gd, "group_size": Wg, "K": d.K, "R": d.R, "A": d.A, "V": d.V,
           "seq_length": d.L, "reps": reps, "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        with step_limit("diversity"):
            fw, cp = {}, {}
            for lam in LAMBDAS:
                fw[str(lam)], cp[str(lam)] = distinct(diverse(lam)[0].reshape(B * S, N, -1))
            fw["plain"], cp["plain"] = distinct(plain()[0].reshape(B * S, N, -1))
            out["first_words"], out["captions"] = fw, cp
        td, tp = [], []
        for r in range(runs):                                     # alternated: diverse, plain, diverse, plain, ...
            with step_limit("run %d diverse" % r):
                td.append(event_ms(diverse, reps))
            with step_limit("run %d plain" % r):
                tp.append(event_ms(plain, reps))
    out["diverse_ms"] = [round(v, 3) for v in td]
    out["plain_ms"] = [round(v, 3) for v in tp]
    out["diverse_ms_spread"] = round(max(td) - min(td), 3)
    out["plain_ms_spread"] = round(max(tp) - min(tp), 3)
    out["ratio"] = round(mean(td) / mean(tp), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
