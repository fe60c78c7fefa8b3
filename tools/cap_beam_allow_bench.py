#!/usr/bin/env python3
"""Timing of the captioner's beam search whose words must follow a POS template (docs/CAPTION_ALLOW.md).  One process; every GPU step
runs under a time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints
one JSON line and writes it to profiles/cap_beam_allow_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26, R 512,
A 1536, V 20000, seq_length 20), beam width W (5), S rows per video, `runs` (3) alternated runs of the constrained and the
unconstrained search on the same inputs, each the best of `reps` (20) calls by device events around the WHOLE call (encoder included;
both return without a host synchronisation):

  allowed_ms[S]         SAModel.beam_captions_allowed (include/xgate_beam_allow.h) under templates of 6 .. 12 single tags
  free_ms[S]            SAModel.beam_captions_per_video (include/xgate_beam_control.h).  The yardstick: this work leaves it as it was
  *_spread[S]           max - min over the runs
  ratio[S]              mean allowed_ms / mean free_ms
  adherent[S]           live beams (score > -500) whose every token is allowed at its position, of all live beams
  mean_words[S]         mean number of words of the best beam under the constraint / without it

The table: 14 categories over V words with the shares SHARES (word 0 alone in category 0, word 1 in category 1), drawn with a fixed
seed; a template's tags are drawn with the same shares over categories 2 .. 13.

  usage: cap_beam_allow_bench.py [reps] [--s 1,4,8] [--w 5] [--runs 3] [--out PATH | --no-out] [--profile-pass]
  --profile-pass: no timing; three calls of each search at every S, for a kernel trace taken around this process
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import paramgen as pg  # noqa: E402
from tests.util import CFG, make_model  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402

B = 64
# share of the vocabulary per category 1 .. 13 (unknown, verb, noun, adjective, adverb, conjunction, pronoun, preposition, determiner,
# particle / modal, number, symbol, interjection): nouns about half of a caption vocabulary, verbs a fifth, adjectives a seventh
SHARES = [0.04, 0.20, 0.50, 0.14, 0.05, 0.005, 0.01, 0.02, 0.01, 0.005, 0.01, 0.005, 0.005]


def make_table(V, seed=0):
    rng = np.random.RandomState(seed)
    p = np.array(SHARES) / sum(SHARES)
    t = (1 + rng.choice(len(p), size=V, p=p)).astype(np.uint8)
    t[0], t[1] = 0, 1
    return t


def make_templates(G, L, seed=1):
    """(G,L) int64 tags: 6 .. 12 tags of categories 2 .. 13 drawn by SHARES, then the end tag 0."""
    rng = np.random.RandomState(seed)
    p = np.array(SHARES[1:]) / sum(SHARES[1:])
    t = np.zeros((G, L), np.int64)
    for g in range(G):
        n = rng.randint(6, 13)
        t[g, :n] = 2 + rng.choice(len(p), size=n, p=p)
    return t


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ss = [int(v) for v in argv[argv.index("--s") + 1].split(",")] if "--s" in argv else [1, 4, 8]
    W = int(argv[argv.index("--w") + 1]) if "--w" in argv else 5
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_beam_allow_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_beam_allow_bench needs a GPU")
    from controllable_xgating_amd import allow_masks, template_adherence
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    assert d.L >= 13
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = {S: torch.from_numpy(pg.uniform("pos_feats_s", (B * S, d.R), 3, -1.0, 1.0)).cuda().reshape(B, S, d.R) for S in ss}
        wc = torch.from_numpy(make_table(d.V)).cuda()
        allow = {S: allow_masks(torch.from_numpy(make_templates(B * S, d.L)).reshape(B, S, d.L), d.L).cuda() for S in ss}

    def allowed(S):
        return m.beam_captions_allowed(*f, pos[S], wc, allow[S], beam_size=W)

    def free(S):
        return m.beam_captions_per_video(*f, pos[S], beam_size=W)

    if "--profile-pass" in argv:
        with torch.no_grad():
            for S in ss:
                with step_limit("profile pass S=%d" % S):
                    for _ in range(3):
                        allowed(S)
                        free(S)
                    torch.cuda.synchronize()
        return
    out = {"tool": "cap_beam_allow_bench", "B": B, "W": W, "K": d.K, "R": d.R, "A": d.A, "V": d.V, "seq_length": d.L, "reps": reps,
           "runs": runs, "shares": SHARES, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    with torch.no_grad():
        for S in ss:
            with step_limit("beams S=%d" % S):
                seq, _, score = allowed(S)
                live = score > -500
                adh = template_adherence(seq, allow[S], wc)
                out["adherent[%d]" % S] = "%d of %d" % (int((adh & live).sum()), int(live.sum()))
                words = lambda s: float((s[:, :, 0] != 0).long().cumprod(2).sum(2).float().mean())     # noqa: E731
                out["mean_words[%d]" % S] = [round(words(seq), 2), round(words(free(S)[0]), 2)]
            ta, tf = [], []
            for r in range(runs):                                 # alternated: allowed, free, allowed, free, ...
                with step_limit("run %d allowed S=%d" % (r, S)):
                    ta.append(event_ms(lambda: allowed(S), reps))
                with step_limit("run %d free S=%d" % (r, S)):
                    tf.append(event_ms(lambda: free(S), reps))
            out["allowed_ms[%d]" % S] = [round(v, 3) for v in ta]
            out["free_ms[%d]" % S] = [round(v, 3) for v in tf]
            out["allowed_ms_spread[%d]" % S] = round(max(ta) - min(ta), 3)
            out["free_ms_spread[%d]" % S] = round(max(tf) - min(tf), 3)
            out["ratio[%d]" % S] = round(mean(ta) / mean(tf), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
