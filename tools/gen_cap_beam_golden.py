#!/usr/bin/env python3
"""Generate the captioner's beam-search fixtures tests/golden/cap_beam_*.npz from the REFERENCE itself.

Runs only where the reference tree exists, with the shims and `build_ref` of tools/gen_golden.py, as its own process.  For every
case of tests/cap_beam_oracle.BEAM_CASES it runs the reference's ``model.sample(.., {"beam_size": W})`` in eval mode on the seeded
weights and inputs and records outputs only (a few KB each):

    tokens (B,L,W)       the tokens the reference feeds after every step, in every slot: an instance-level wrapper around
                         get_logprobs_state records its `it`
    top_lp, top_ix (B,L,W,W+1)
                         per step and slot the W + 1 largest log-probabilities AFTER the -1000 on UNK (index 1) with their word
                         indices, lower word first on ties (a forward hook on `logit`; the full V is not stored)
    ref_seq, ref_logps   (B,W,L) 'seq' / 'logps' of the reference's returned done_beams.  Under a torch that returns a 0-dim VIEW
                         for ``beam_logprobs_sum[vix]`` the reference overwrites every stored 'p' with -1000 on its next line, so
                         its final sort is a no-op and these are the first W COMPLETIONS; 'p' is therefore not stored
    done_t, done_slot, done_score (B,N), done_n (B,)
                         the done list in completion order, derived here by steps 3-5 of include/xgate_beam.h
                         (tests/pos_beam_oracle.VideoSearch)
    margin (B,)          the smallest gap that decided a step (tests/pos_beam_oracle.step_margin) over the steps that select at
                         least one candidate with p > -500

It asserts that the replay of steps 3-5 reproduces the recorded tokens of every step and slot, that the reference's returned beams
are the head of the replay's completion-ordered done list, that tiny_w3 and eos_w3 pin at least 4 of their 5 videos, and that a
second run gives byte-identical files.

    python tools/gen_cap_beam_golden.py        # writes tests/golden/cap_beam_*.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cap_beam_oracle as cbo  # noqa: E402
from tests import pos_beam_oracle as pbo  # noqa: E402
from tools import gen_golden as gg  # noqa: E402
from tools.gen_pos_beam_golden import npz_bytes  # noqa: E402

SUPPRESS = 1                                  # CaptionModel.py:94
MIN_PINNED = {"tiny_w3": 4, "eos_w3": 4}


def gen_case(ref, name):
    d, P, x, W = cbo.case_setup(name)
    model = gg.build_ref(ref, d, P)
    model.eval()
    xt = gg.tt(x)
    its, tops = [], []
    inner = model.get_logprobs_state

    def recording(it, *a, **k):
        its.append(it.detach().clone().numpy())
        return inner(it, *a, **k)

    def hook(m, i, o):
        lp = torch.log_softmax(o.detach(), 1).numpy().copy()
        lp[:, SUPPRESS] -= np.float32(1000)
        ix = np.argsort(-lp, axis=1, kind="stable")[:, :W + cbo.TOPK_EXTRA]
        tops.append((np.take_along_axis(lp, ix, 1), ix))

    model.get_logprobs_state = recording
    h = model.logit.register_forward_hook(hook)
    with gg.quiet(), torch.no_grad():
        model.sample(xt["feats_rgb"], xt["feats_opfl"], xt["feat_mask"], xt["pos_feats"], {"beam_size": W})
    h.remove()
    B, L, k = d.B, d.L, W + cbo.TOPK_EXTRA
    assert len(its) == B * L and len(tops) == B * (L + 1), (len(its), len(tops))
    tokens = np.array(its).reshape(B, L, W).astype(np.int64)
    top_lp = np.array([t[0] for t in tops]).reshape(B, L + 1, W, k)[:, :L].astype(np.float32)     # (the last step's state is never merged)
    top_ix = np.array([t[1] for t in tops]).reshape(B, L + 1, W, k)[:, :L].astype(np.int64)
    ref_seq = np.array([[e["seq"].numpy() for e in model.done_beams[b]] for b in range(B)]).astype(np.int64)
    ref_lps = np.array([[e["logps"].numpy() for e in model.done_beams[b]] for b in range(B)]).astype(np.float32)
    assert ref_seq.shape == (B, W, L)
    done, margin = [], np.zeros(B, np.float64)
    for b in range(B):
        vs = pbo.VideoSearch(W, L, np.float32)
        for t in range(L):
            _, c = vs.feed(cbo.sparse_rows(top_lp[b, t], top_ix[b, t]))
            assert np.array_equal(c, tokens[b, t]), (name, b, t, c, tokens[b, t])
        for r in range(W):                                                          # the first W completions, in order
            assert np.array_equal(vs.done[r]["seq"], ref_seq[b, r]) and np.array_equal(vs.done[r]["logps"], ref_lps[b, r]), (name, b, r)
        done.append(vs.done)
        margin[b] = vs.margin
    N = max(len(v) for v in done)
    g = dict(tokens=tokens, top_lp=top_lp, top_ix=top_ix, ref_seq=ref_seq, ref_logps=ref_lps, margin=margin,
             done_n=np.array([len(v) for v in done], np.int64), done_t=np.full((B, N), -1, np.int64),
             done_slot=np.full((B, N), -1, np.int64), done_score=np.zeros((B, N), np.float32))
    for b, v in enumerate(done):
        for i, e in enumerate(v):
            g["done_t"][b, i], g["done_slot"][b, i], g["done_score"][b, i] = e["t"], e["slot"], e["score"]
    early = [int(sum(1 for e in v if e["t"] < L - 1)) for v in done]
    print("cap_beam_%s: W %d  completions %s  early %s  margins %s" % (name, W, g["done_n"].tolist(), early,
                                                                         " ".join("%.1e" % m for m in margin)))
    assert int((margin >= cbo.MARGIN).sum()) >= MIN_PINNED.get(name, 0), (name, margin)
    return npz_bytes(g)


def main():
    if not os.path.isdir(gg.REF):
        print("reference not present; nothing to do")
        return 0
    os.makedirs(gg.GOLD, exist_ok=True)
    torch.set_num_threads(8)
    ref = gg.import_reference()
    for name in cbo.BEAM_CASES:
        first = gen_case(ref, name)
        assert gen_case(ref, name) == first, name + ": two runs differ"
        with open(os.path.join(gg.GOLD, "cap_beam_%s.npz" % name), "wb") as f:
            f.write(first)
    return 0


if __name__ == "__main__":
    sys.exit(main())
