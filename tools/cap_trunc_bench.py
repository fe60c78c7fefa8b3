#!/usr/bin/env python3
"""Timing of truncated (top-k / nucleus) caption sampling (docs/CAPTION_TRUNCATED.md).  One process; every GPU step runs under a
time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON
line and writes it to profiles/cap_trunc_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26, R 512, A 1536,
V 20000, seq_length 20) under S = 8 rows per video, the same inputs and the same uniforms for every call, `runs` (3) alternated
runs, each the best of `reps` (20) calls by device events around the WHOLE call (encoder included; none synchronises the host):

  plain_ms              SAModel.sample_per_video in sampled mode (include/xgate_control.h).  The yardstick: this work leaves it
                        as it was
  top_p_ms, top_k_ms,   SAModel.sample_truncated_per_video (include/xgate_truncate.h) with top_p 0.9, with top_k 50, and with
  both_ms               both; no statistics asked for
  *_spread              max - min over the runs;  *_ratio: mean of the setting / mean plain_ms
  *_kept                mean size of the kept set over the live steps
  *_tail                share of the rows with a word whose LAST live word lies outside the top 50 of its step: the rank is
                        counted in float64 over the model's own teacher-forced log-probabilities of that caption (SAModel
                        forward, fp32 on the device) -- the junk last word that truncation is there to remove
  *_words               mean number of words per row

  usage: cap_trunc_bench.py [reps] [--s 8] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; three calls of every setting, for a kernel trace taken around this process
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
TOP = 50
SETTINGS = {"top_p": dict(top_p=0.9), "top_k": dict(top_k=TOP), "both": dict(top_k=TOP, top_p=0.9)}


def tail_share(m, f, pos, seq, S, chunk=8):
    """(share of rows whose last live word has rank >= TOP, mean words per row) for captions seq (B,S,L)."""
    Bv, _, L = seq.shape
    outside = rows = words = 0
    for b0 in range(0, Bv, chunk):
        b1 = min(Bv, b0 + chunk)
        s = seq[b0:b1].reshape(-1, L)
        n = (s > 0).long().cumprod(1).sum(1)                      # words before the end token
        fed = torch.cat([torch.zeros_like(s[:, :1]), s], 1)       # <bos>, then the caption
        logp, _ = m(*[t[b0:b1].repeat_interleave(S, 0) for t in f], pos[b0:b1].reshape(-1, pos.shape[-1]), fed, torch.ones_like(fed, dtype=torch.float32))
        has = n > 0
        j = (n - 1).clamp(min=0)
        j = j.clamp(max=logp.shape[1] - 1)
        r = torch.arange(s.shape[0], device=s.device)
        row = logp[r, j].double()                                 # the step that chose the last word
        rank = (row > row[r, s[r, j]].unsqueeze(1)).sum(1)
        outside += int(((rank >= TOP) & has).sum())
        rows += int(has.sum())
        words += int(n.sum())
    return round(outside / max(rows, 1), 4), round(words / (Bv * S), 2)


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    S = int(argv[argv.index("--s") + 1]) if "--s" in argv else 8
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_trunc_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_trunc_bench needs a GPU")
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = torch.from_numpy(pg.uniform("pos_feats_s", (B * S, d.R), 3, -1.0, 1.0)).cuda().reshape(B, S, d.R)
        u = torch.from_numpy(pg.uniform("u", (d.L + 1, B * S), 3)).cuda()

    def plain():
        return m.sample_per_video(*f, pos, {"sample_max": 0, "uniforms": u, "async": True})

    def trunc(name, stats=False):
        return m.sample_truncated_per_video(*f, pos, uniforms=u, return_stats=stats, trim=False, **SETTINGS[name])

    calls = dict({"plain": plain}, **{k: (lambda k=k: trunc(k)) for k in SETTINGS})
    if "--profile-pass" in argv:
        with torch.no_grad():
            for name, fn in calls.items():
                with step_limit("profile pass " + name):
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
        return
    out = {"tool": "cap_trunc_bench", "B": B, "S": S, "K": d.K, "R": d.R, "A": d.A, "V": d.V, "seq_length": d.L, "reps": reps, "runs": runs,
           "top": TOP, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        with step_limit("captions and their statistics"):
            out["plain_tail"], out["plain_words"] = tail_share(m, f, pos, plain()[0], S)
            out["plain_kept"] = d.V
            for name in SETTINGS:
                seq, _, _, kept, _ = trunc(name, stats=True)
                live = torch.cat([torch.ones_like(seq[..., :1], dtype=torch.bool), seq[..., :-1] > 0], 2)
                out[name + "_kept"] = round(float(kept[live].float().mean()), 1)
                out[name + "_tail"], out[name + "_words"] = tail_share(m, f, pos, seq, S)
        ms = {k: [] for k in calls}
        for r in range(runs):                                     # alternated: plain, top_p, top_k, both, plain, ...
            for name, fn in calls.items():
                with step_limit("run %d %s" % (r, name)):
                    ms[name].append(event_ms(fn, reps))
    for name, v in ms.items():
        out[name + "_ms"] = [round(t, 3) for t in v]
        out[name + "_ms_spread"] = round(max(v) - min(v), 3)
        if name != "plain":
            out[name + "_ratio"] = round(mean(v) / mean(ms["plain"]), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
