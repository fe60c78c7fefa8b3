#!/usr/bin/env python3
"""Timing of the SCST rollout pair under train-mode dropout (docs/SCST_DROPOUT.md): one iteration = SAModel.sample_pair +
RewardCriterion + backward at BASELINE.json configs[2] (B 64, K 26, R 512, A 1536, E 468, V 20000, seq_length 30, fp32) with
drop_prob_lm = 0.5, in its two forms:

  two_call_ms    sample_pair as it is at p > 0: two m-row rollouts, one after the other (2 L dependent steps)
  one_pass_ms    sample_pair(..., {"one_pass": True}): one 2m-row rollout with a dropout seed per half (L steps), the encoder
                 once per seed (include/xgate_pair.h)

One process, the two forms ALTERNATE iteration by iteration after `warmup` (5) iterations of each, `reps` (30, at least 20)
timed iterations each, every iteration between two device events and waited for.  Both forms draw from the same uniforms; the
seeds advance with the model's counter as in training.  Prints one JSON line (and writes it to --out): per form the median, the
minimum, the maximum and the quartiles; `spread` = max - min of the timed iterations; ratio = median two_call / median one_pass;
beats_spread = the median gain exceeds the two-call form's own spread.  Every GPU step runs under a time limit of its own.

  usage: scst_drop_bench.py [reps] [--warmup 5] [--out PATH | --no-out]
"""
from __future__ import annotations

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import synth_inputs  # noqa: E402
from tools.pos_control_bench import step_limit  # noqa: E402

CFG = dict(B=64, K=26, R=512, A=1536, E=468, V=20000, C=14, L=30, F1=1536, F2=1024)
P_DROP = 0.5


def main():
    argv = sys.argv[1:]
    reps = max(20, int(argv[0])) if argv and argv[0].isdigit() else 30
    warmup = int(argv[argv.index("--warmup") + 1]) if "--warmup" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "scst_drop_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("scst_drop_bench needs a GPU")
    from controllable_xgating_amd import RewardCriterion, SAModel, make_opt
    dev = torch.device("cuda:0")
    c = CFG
    with step_limit("model and inputs"):
        opt = make_opt(None, vocab_size=c["V"], seq_length=c["L"], drop_prob_lm=P_DROP, precision="fp32", rnn_size=c["R"],
                       att_size=c["A"], input_encoding_size=c["E"], feat_size=c["F1"], feat_size2=c["F2"])
        torch.manual_seed(0)
        model = SAModel(opt).to(dev)
        model.train()
        x = synth_inputs(c["B"], c["K"], c["L"], c["V"], c["R"], c["F1"], c["F2"], c["C"], seed=0, device=dev)
        reward = torch.randn(c["B"], 1, generator=torch.Generator().manual_seed(7)).to(dev)
        uni = torch.rand(c["L"] + 1, c["B"], generator=torch.Generator().manual_seed(11)).to(dev)
    crit = RewardCriterion()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def iteration(one_pass):
        o = {"uniforms": uni}
        if one_pass:
            o["one_pass"] = True
        a.record()
        gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], o)
        loss = crit(slp, gen, reward, n=n[:1])
        loss.backward()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    with step_limit("warm-up"):
        for _ in range(warmup):
            iteration(False)
            iteration(True)
    t = {False: [], True: []}
    for r in range(reps):
        with step_limit("timed iteration %d" % r):
            for form in (False, True):
                t[form].append(iteration(form))

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "q1": round(q[0], 3),
                "q3": round(q[2], 3), "spread": round(max(v) - min(v), 3)}

    two, one = stats(t[False]), stats(t[True])
    out = dict(tool="scst_drop_bench", reps=reps, warmup=warmup, drop_prob_lm=P_DROP, precision="fp32", two_call_ms=two, one_pass_ms=one,
               ratio=round(two["median"] / one["median"], 3), gain_ms=round(two["median"] - one["median"], 3),
               beats_spread=bool(two["median"] - one["median"] > two["spread"]),
               library=os.path.basename(os.environ.get("XG_LIBRARY", "libxgate_hip.so")), **{k: v for k, v in c.items()})
    line = json.dumps(out)
    print(line)
    if "--no-out" not in argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
