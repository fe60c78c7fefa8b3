#!/usr/bin/env python3
"""Timing of the fused teacher-forced loss under scheduled sampling (docs/CAPTION_SS.md).  One process; every GPU step runs under a
time limit of its own (a step that overruns it ends the process with a traceback, and nothing more is started).  Prints one JSON line
and writes it to profiles/cap_ss_bench.json (--out).  BASELINE.json configs[1] layer sizes (K 26, R 512, A 1536, V 20000, seq_length
20), 128 caption rows -- as 128 rows and as 32 videos x 4 captions --, train mode, drop_prob_lm 0, ss_prob 0.25, fixed uniforms, no
classifier term, gradients accumulated into the bound flat buffer as the trainer has it.  `runs` (3) alternated runs of the three
lines, each the best of `reps` (10) calls of forward + backward WITHOUT the optimizer step, by device events around the whole call,
every shape warmed first:

  unfused_ms[S]          (a) model() + LanguageModelCriterion + backward() under ss_prob: the path that honoured ss_prob before
                         (32x4: on repeat_interleave'd inputs, the repeat inside the timed region)
  fused_ms[S]            (b) SAModel.xe_loss_ss / xe_loss_ss_per_video + backward (include/xgate_ss.h)
  teacher_ms[S]          (c) SAModel.xe_loss / xe_loss_per_video + backward at ss_prob 0: the floor that teacher forcing sets
  *_spread[S]            max - min over the runs
  faster_every_run[S]    fused_ms < unfused_ms in every alternated run;  faster_by_more_than_spread[S]: ... by more than unfused_ms_spread
  ratio_unfused[S]       mean unfused_ms / mean fused_ms;  ratio_teacher[S]: mean fused_ms / mean teacher_ms, what scheduled sampling costs
  unfused_peak_bytes[S], fused_peak_bytes[S]   torch.cuda.max_memory_allocated over two calls of the line, measured from a reset peak
  rows_tokens_differ[S]  share of rows whose fed tokens differ between (a) and (b); (a)'s are formed from its log-probs by the rule
  loss_unfused[S], loss_fused[S]

  usage: cap_ss_bench.py [reps] [--shapes 128x0,32x4] [--runs 3] [--out PATH | --no-out] [--profile-pass [--only unfused|fused|teacher]]
  --profile-pass: no timing; two calls of each line (of the named one) at every shape, for a kernel trace taken around this process
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

SS_PROB = 0.25


def main():
    argv = sys.argv[1:]
    reps = int(argv[0]) if argv and argv[0].isdigit() else 10
    shapes = argv[argv.index("--shapes") + 1] if "--shapes" in argv else "128x0,32x4"
    shapes = [tuple(int(v) for v in s.split("x")) for s in shapes.split(",")]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    only = argv[argv.index("--only") + 1] if "--only" in argv else None
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cap_ss_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cap_ss_bench needs a GPU")
    from controllable_xgating_amd import LanguageModelCriterion
    d0 = pg.make_dims(**CFG["c1"])
    T = d0.L + 1
    crit = LanguageModelCriterion()
    with step_limit("model"):
        m = make_model(d0, train=True)
        m.flat_grads()                                            # gradients accumulate in place, as under train.ClipAdam

    def inputs(B, Q):
        M = B * max(Q, 1)
        x = pg.make_inputs(d0._replace(B=B), seed=3)
        r = x if Q == 0 else pg.make_inputs(d0._replace(B=M), seed=4)
        f = [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
        rows = [torch.from_numpy(r[k]).cuda() for k in ("pos_feats", "seq", "seq_mask")]
        g = torch.Generator(device="cuda").manual_seed(5)
        u = (torch.rand(T, M, device="cuda", generator=g), torch.rand(T, M, device="cuda", generator=g))
        return f, rows, u

    def unfused(f, rows, u, B, Q):
        m.ss_prob, m.ss_uniforms = SS_PROB, u
        ff = f if Q == 0 else [t.repeat_interleave(Q, 0) for t in f]
        logp, _ = m(*ff, *rows)
        loss = crit(logp, rows[1], rows[2])
        loss.backward()
        return loss, logp

    def fused(f, rows, u, B, Q):
        m.ss_prob, m.ss_uniforms = SS_PROB, u
        if Q == 0:
            loss = m.xe_loss_ss(*f, *rows)
        else:
            loss = m.xe_loss_ss_per_video(*f, rows[0].reshape(B, Q, -1), rows[1].reshape(B, Q, T), rows[2].reshape(B, Q, T))
        loss.backward()
        return loss, None

    def teacher(f, rows, u, B, Q):
        m.ss_prob = 0.0
        if Q == 0:
            loss = m.xe_loss(*f, *rows)
        else:
            loss = m.xe_loss_per_video(*f, rows[0].reshape(B, Q, -1), rows[1].reshape(B, Q, T), rows[2].reshape(B, Q, T))
        loss.backward()
        return loss, None

    lines = (("unfused", unfused), ("fused", fused), ("teacher", teacher))

    def fed_by_the_rule(logp, seq, u):
        """(T, M) fed tokens of the un-fused path, formed from ITS log-probs: the first index whose running float64 sum of exp(logp)
        exceeds u_tok times the total, where u_sel < ss_prob."""
        fed = seq.t().clone()
        for t in range(1, T):
            cdf = logp[:, t - 1].double().exp().cumsum(1)
            tk = torch.searchsorted(cdf, (u[1][t].double() * cdf[:, -1]).unsqueeze(1), right=True).squeeze(1).clamp(max=logp.shape[2] - 1)
            fed[t] = torch.where(u[0][t] < SS_PROB, tk, fed[t])
        return fed

    if "--profile-pass" in argv:
        for B, Q in shapes:
            f, rows, u = inputs(B, Q)
            with step_limit("profile pass %dx%d" % (B, Q)):
                for _ in range(2):
                    for name, fn in lines:
                        if only in (None, name):
                            fn(f, rows, u, B, Q)
                torch.cuda.synchronize()
        return
    out = {"tool": "cap_ss_bench", "K": d0.K, "R": d0.R, "A": d0.A, "V": d0.V, "seq_length": d0.L, "ss_prob": SS_PROB, "reps": reps,
           "runs": runs, "library": os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so"))}
    mean = lambda v: sum(v) / len(v)                              # noqa: E731
    for B, Q in shapes:
        key = "%dx%d" % (B, Q)
        f, rows, u = inputs(B, Q)
        with step_limit("warm-up and tokens " + key):
            for _, fn in lines:
                fn(f, rows, u, B, Q)
            la, logp = unfused(f, rows, u, B, Q)
            fed_a = fed_by_the_rule(logp.detach(), rows[1], u)
            del logp
            lb, _ = fused(f, rows, u, B, Q)
            fed_b = m.last_ss_tokens
            torch.cuda.synchronize()
            out["loss_unfused[%s]" % key], out["loss_fused[%s]" % key] = float(la.item()), float(lb.item())
            out["rows_tokens_differ[%s]" % key] = float((fed_a != fed_b).any(0).float().mean().item())
            out["fed_tokens_drawn[%s]" % key] = float((fed_b != rows[1].t()).float().mean().item())
            del la, lb
        for name, fn in lines[:2]:
            with step_limit("peak memory %s %s" % (name, key)):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                for _ in range(2):
                    fn(f, rows, u, B, Q)
                torch.cuda.synchronize()
                out["%s_peak_bytes[%s]" % (name, key)] = int(torch.cuda.max_memory_allocated())
        t = {name: [] for name, _ in lines}
        for r in range(runs):                                     # alternated: unfused, fused, teacher, unfused, ...
            for name, fn in lines:
                with step_limit("run %d %s %s" % (r, name, key)):
                    t[name].append(event_ms(lambda: fn(f, rows, u, B, Q), reps))
        for name, _ in lines:
            out["%s_ms[%s]" % (name, key)] = [round(v, 3) for v in t[name]]
            out["%s_ms_spread[%s]" % (name, key)] = round(max(t[name]) - min(t[name]), 3)
        spread = max(t["unfused"]) - min(t["unfused"])
        out["faster_every_run[%s]" % key] = all(b_ < a_ for a_, b_ in zip(t["unfused"], t["fused"]))
        out["faster_by_more_than_spread[%s]" % key] = all(a_ - b_ > spread for a_, b_ in zip(t["unfused"], t["fused"]))
        out["ratio_unfused[%s]" % key] = round(mean(t["unfused"]) / mean(t["fused"]), 3)
        out["ratio_teacher[%s]" % key] = round(mean(t["fused"]) / mean(t["teacher"]), 3)
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
