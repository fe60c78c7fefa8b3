#!/usr/bin/env python3
"""Timing of the captioner's beam search under decoding rules (docs/CAPTION_RULES.md).  One process; every GPU step runs under a time
limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line and
writes it to profiles/cap_beam_rules_bench.json (--out).  At B 64 videos of BASELINE.json configs[1] (K 26, R 512, A 1536, V 20000,
seq_length 20), beam width W (5), S rows per video: `runs` (3) rounds in which EVERY line below is timed once, one after the other
on the same inputs (interleaved, so a drift of the device meets them all), each the best of `reps` (20) calls by device events
around the WHOLE call (encoder included; all return without a host synchronisation):

  free_ms[S]            SAModel.beam_captions_per_video (include/xgate_beam_control.h): the yardstick, code this work leaves as it was
  allowed_ms[S]         SAModel.beam_captions_allowed (include/xgate_beam_allow.h) under templates of 6 .. 12 single tags: likewise
  off_ms[S], off_m_ms[S]    SAModel.beam_captions_ruled with every rule off, without / with those masks
  n3_ms[S], n3_m_ms[S]      ... at no_repeat_ngram 3
  all_ms[S], all_m_ms[S]    ... at no_repeat_ngram 3, min_length 5, 17 bad endings and length_scale_table(L, 1.0)
  *_spread[S]           max - min over the rounds
  trigram_share[S]      share of live beams (score > -500) that hold a trigram twice: free, n3, all
  mean_words[S]         mean number of words of the best beam: free, n3, all

The vocabulary of the bench has no words: the 17 bad endings are the indices 2 .. 18, standing for data.BAD_ENDINGS.  Table and
templates: tools/cap_beam_allow_bench.py.

  usage: cap_beam_rules_bench.py [reps] [--s 1,8] [--w 5] [--runs 3] [--out PATH | --no-out]
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
from tools.cap_beam_allow_bench import B, make_table, make_templates  # noqa: E402
from tools.pos_bench import event_ms  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402

BAD = list(range(2, 19))


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 20
    ss = [int(v) for v in argv[argv.index("--s") + 1].split(",")] if "--s" in argv else [1, 8]
    W = int(argv[argv.index("--w") + 1]) if "--w" in argv else 5
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_beam_rules_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_beam_rules_bench needs a GPU")
    from controllable_xgating_amd import allow_masks, length_scale_table, repeated_ngrams
    d = pg.make_dims(**dict(CFG["c1"], B=B))
    with step_limit("model and inputs"):
        m = make_model(d, train=False)
        x = pg.make_inputs(d, seed=3)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        pos = {S: torch.from_numpy(pg.uniform("pos_feats_s", (B * S, d.R), 3, -1.0, 1.0)).cuda().reshape(B, S, d.R) for S in ss}
        wc = torch.from_numpy(make_table(d.V)).cuda()
        allow = {S: allow_masks(torch.from_numpy(make_templates(B * S, d.L)).reshape(B, S, d.L), d.L).cuda() for S in ss}
        scale = length_scale_table(d.L, 1.0)
    n3 = dict(no_repeat_ngram=3)
    full = dict(no_repeat_ngram=3, min_length=5, bad_endings=BAD, length_scale=scale)

    def ruled(S, masks, **kw):
        if masks:
            kw.update(word_cat=wc, allow=allow[S])
        return m.beam_captions_ruled(*f, pos[S], beam_size=W, **kw)

    lines = {
        "free": lambda S: m.beam_captions_per_video(*f, pos[S], beam_size=W),
        "allowed": lambda S: m.beam_captions_allowed(*f, pos[S], wc, allow[S], beam_size=W),
        "off": lambda S: ruled(S, False), "off_m": lambda S: ruled(S, True),
        "n3": lambda S: ruled(S, False, **n3), "n3_m": lambda S: ruled(S, True, **n3),
        "all": lambda S: ruled(S, False, **full), "all_m": lambda S: ruled(S, True, **full),
    }
    out = {"tool": "cap_beam_rules_bench", "B": B, "W": W, "K": d.K, "R": d.R, "A": d.A, "V": d.V, "seq_length": d.L, "reps": reps,
           "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    with torch.no_grad():
        for S in ss:
            with step_limit("beams S=%d" % S):
                share, words = [], []
                for name in ("free", "n3", "all"):
                    res = lines[name](S)
                    seq, score = res[0], res[2]
                    live = score > -500
                    share.append(round(float((repeated_ngrams(seq, 3) & live).sum()) / max(1, int(live.sum())), 4))
                    words.append(round(float((seq[:, :, 0] != 0).long().cumprod(2).sum(2).float().mean()), 2))
                out["trigram_share[%d]" % S], out["mean_words[%d]" % S] = share, words
            times = {k: [] for k in lines}
            for r in range(runs):                                 # interleaved: every line once per round
                for name, fn in lines.items():
                    with step_limit("round %d %s S=%d" % (r, name, S)):
                        times[name].append(event_ms(lambda: fn(S), reps))
            for name, t in times.items():
                out["%s_ms[%d]" % (name, S)] = [round(v, 3) for v in t]
                out["%s_ms_spread[%d]" % (name, S)] = round(max(t) - min(t), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
