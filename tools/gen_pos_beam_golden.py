#!/usr/bin/env python3
"""Generate the POS beam-search fixtures tests/golden/pos_beam_*.npz from the REFERENCE itself.

Runs only where the reference tree exists, with the shims and `build_ref` of tools/gen_pos_golden.py, as its own process.  For every
case of tests/pos_beam_oracle.BEAM_CASES it runs the reference's ``model.sample(.., {"beam_size": W})`` on the seeded weights and
inputs of tests/pos_oracle.GOLDEN_CASES and records outputs only:

    tokens (B,L,W)       the tokens the reference feeds after every step, in every slot: an instance-level wrapper around
                         get_logprobs_state records its `it`
    logps (B,L,W,C)      the log-probabilities every step's merge was made from (before the -1000 on category 1): a forward hook
                         on `logit`
    ref_seq, ref_logps   (B,W,L) 'seq' / 'logps' of the reference's returned done_beams.  Under a torch that returns a 0-dim VIEW
                         for ``beam_logprobs_sum[vix]`` the reference overwrites every stored 'p' with -1000 on its next line, so
                         its final sort is a no-op and these are the first W COMPLETIONS; 'p' is therefore not stored
    done_t, done_slot, done_score (B,N), done_n (B,)
                         the done list in completion order, derived here from `logps` by steps 3-5 of include/xgate_pos_beam.h
                         (tests/pos_beam_oracle.VideoSearch)
    margin (B,)          the smallest gap that decided a step (tests/pos_beam_oracle.step_margin) over the steps that select at
                         least one candidate with p > -500

It asserts that the replay of steps 3-5 reproduces the recorded tokens of every step and slot, that the reference's returned beams
are the head of the replay's completion-ordered done list, and that a second run gives byte-identical files.

    python tools/gen_pos_beam_golden.py        # writes tests/golden/pos_beam_*.npz
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pos_beam_oracle as pbo  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tools import gen_pos_golden as gpg  # noqa: E402

SUPPRESS = 1                                  # CaptionModel.py:92


def npz_bytes(arrays):
    """A compressed .npz with fixed member dates: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def gen_case(ref, name):
    case, W = pbo.BEAM_CASES[name]
    cfg, kw, eos = po.GOLDEN_CASES[case]
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **dict(kw))
    model, _, _ = gpg.build_ref(ref, d, P, run)
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    its, logps = [], []
    inner = model.get_logprobs_state

    def recording(it, *a, **k):
        its.append(it.detach().clone().numpy())
        return inner(it, *a, **k)

    model.get_logprobs_state = recording
    hook = model.logit.register_forward_hook(lambda m, i, o: logps.append(torch.log_softmax(o.detach(), 1).numpy().copy()))
    with gpg.quiet(), torch.no_grad():
        model.sample(fr, fo, fm, {"beam_size": W})
    hook.remove()
    B, L, C = d.B, d.L, d.C
    assert len(its) == B * L and len(logps) == B * (L + 1)
    tokens = np.array(its).reshape(B, L, W).astype(np.int64)
    lp = np.array(logps).reshape(B, L + 1, W, C)[:, :L].astype(np.float32)       # (the last step's state is never merged)
    ref_seq = np.array([[e["seq"].numpy() for e in model.done_beams[b]] for b in range(B)]).astype(np.int64)
    ref_lps = np.array([[e["logps"].numpy() for e in model.done_beams[b]] for b in range(B)]).astype(np.float32)
    assert ref_seq.shape == (B, W, L)
    done, margin = [], np.zeros(B, np.float64)
    for b in range(B):
        vs = pbo.VideoSearch(W, L, np.float32)
        for t in range(L):
            s = lp[b, t].copy()
            s[:, SUPPRESS] -= np.float32(1000)
            _, c = vs.feed(s)
            assert np.array_equal(c, tokens[b, t]), (name, b, t, c, tokens[b, t])
        for k in range(W):                                                          # the first W completions, in order
            assert np.array_equal(vs.done[k]["seq"], ref_seq[b, k]) and np.array_equal(vs.done[k]["logps"], ref_lps[b, k]), (name, b, k)
        done.append(vs.done)
        margin[b] = vs.margin
    N = max(len(v) for v in done)
    g = dict(tokens=tokens, logps=lp, ref_seq=ref_seq, ref_logps=ref_lps, margin=margin,
             done_n=np.array([len(v) for v in done], np.int64), done_t=np.full((B, N), -1, np.int64),
             done_slot=np.full((B, N), -1, np.int64), done_score=np.zeros((B, N), np.float32))
    for b, v in enumerate(done):
        for i, e in enumerate(v):
            g["done_t"][b, i], g["done_slot"][b, i], g["done_score"][b, i] = e["t"], e["slot"], e["score"]
    print("pos_beam_%s: W %d  completions %s  margins %s" % (name, W, g["done_n"].tolist(), " ".join("%.1e" % m for m in margin)))
    return npz_bytes(g)


def main():
    if not os.path.isdir(gpg.REF):
        print("reference not present; nothing to do")
        return 0
    os.makedirs(gpg.GOLD, exist_ok=True)
    torch.set_num_threads(8)
    ref = gpg.import_reference()
    for name in pbo.BEAM_CASES:
        first = gen_case(ref, name)
        assert gen_case(ref, name) == first, name + ": two runs differ"
        with open(os.path.join(gpg.GOLD, "pos_beam_%s.npz" % name), "wb") as f:
            f.write(first)
    return 0


if __name__ == "__main__":
    sys.exit(main())
