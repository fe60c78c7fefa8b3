"""TEST INFRASTRUCTURE ONLY -- the forced POS rollout (include/xgate_pos_control.h) restated in torch on top of tests/pos_oracle.py:
the reference's sample() (pos_src/SAModel.py:136-184) with the torch.max choice replaced by the caller's tag, S templates per video,
row b S + s.  It runs in the dtype and on the device of its inputs (float32 on the CPU against the fixtures, float64 in eager torch
on a GPU as the high-precision reference of tests/test_gpu_pos_control.py)."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from tests import pos_oracle as po

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@torch.no_grad()
def sample_forced(P, run, fr, fo, fm, templates, L):
    """templates (B,S,L) int64 (0-padded).  Returns a dict: tag_logp (B,S,L), states (B,S,L+1,R), masks (B,S,L+1), pos_feats
    (B*S,R), n.  All L + 1 steps run; a finished row holds its state (mask 0)."""
    templates = torch.as_tensor(templates).to(fr.device)
    B, S, Lt = templates.shape
    assert Lt == L
    V, q, h, c = po._prologue(P, run, fr, fo, fm)
    V, q, h, c = (t.repeat_interleave(S, 0) for t in (V, q, h, c))
    tm = templates.reshape(B * S, L)
    M = B * S
    unf = torch.ones(M, dtype=fr.dtype, device=fr.device)
    states, masks, tlp = [], [], []
    logp = None
    for t in range(L + 1):
        if t == 0:
            it = torch.zeros(M, dtype=torch.int64, device=fr.device)
        else:
            it = tm[:, t - 1]
            # counted while the row was unfinished BEFORE this tag: up to and including its first 0
            tlp.append(logp.gather(1, it.unsqueeze(1)).squeeze(1) * unf)
            unf = unf * (it > 0).to(fr.dtype)
        m = unf.unsqueeze(1)
        h, c, logp = po.step(P, V, q, it, m, h, c)
        states.append(h)
        masks.append(unf)
    lead = (tm > 0).to(torch.int64).cumprod(1).sum(1)
    R = h.shape[1]
    return dict(tag_logp=torch.stack(tlp, 1).reshape(B, S, L), states=torch.stack(states, 1).reshape(B, S, L + 1, R),
                masks=torch.stack(masks, 1).reshape(B, S, L + 1), pos_feats=h, n=min(L, int(lead.max())))


def seeded_templates(B, S, L, Cn, seed):
    """(B,S,L) int64: each slot another seeded template with a ragged length.  Slot (0,0) is empty, slot (0,1) -- or (1,0) when
    S = 1 -- is full-length without a 0; the others end after 1 .. L-1 tags and carry junk after their first 0 (which the rollout
    must ignore)."""
    rng = np.random.RandomState(seed)
    t = rng.randint(1, Cn, size=(B, S, L)).astype(np.int64) if Cn > 1 else np.zeros((B, S, L), np.int64)
    lens = rng.randint(1, max(L, 2), size=(B, S))
    lens.reshape(-1)[0] = 0
    if lens.size > 1:
        lens.reshape(-1)[1] = L
    for b in range(B):
        for s in range(S):
            n = int(lens[b, s])
            if n < L:
                t[b, s, n] = 0
    return torch.from_numpy(t), lens


def load_case(name):
    """(d, P, run, x, the reference's outputs) of the fixture tests/golden/pos_<name>.npz."""
    cfg, kw, eos = po.GOLDEN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    g = dict(np.load(os.path.join(GOLD, "pos_%s.npz" % name)))
    return d, po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **kw), g


def golden_template(d, g):
    """The fixture's greedy tokens (B,n) as a (B,1,L) template, and the positions of its seqLogprobs that the forced form
    shares: up to and including a row's first 0 (after it greedy stores a maximum, the forced form 0)."""
    seq, n = g["seq"], int(g["n"])
    tm = np.zeros((d.B, 1, d.L), np.int64)
    tm[:, 0, :n] = seq
    comparable = np.concatenate([np.ones((d.B, 1), bool), np.cumprod(seq[:, :-1] > 0, 1).astype(bool)], 1)
    return tm, comparable


def make_opt(d):
    return argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1, drop_prob_lm=0.0,
                              seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)


def pos_model(d, P, run):
    """PosModel with the seeded parameters and running statistics, on the GPU in eval mode."""
    from controllable_xgating_amd.pos import PosModel
    m = PosModel(make_opt(d))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    return m.cuda().eval()


def cuda_inputs(x):
    return [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]
