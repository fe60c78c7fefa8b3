"""TEST INFRASTRUCTURE ONLY -- the sampled POS rollout (include/xgate_pos_sample.h) restated in torch on top of tests/pos_oracle.py:
the reference's sample() (pos_src/SAModel.py:136-184) with the torch.max choice replaced by the captioner's inverse-CDF draw
(oracle.xgate_oracle.sample_token's rule) from uniforms the caller supplies, S rollouts per video, row b S + s.  It runs in the
dtype and on the device of its inputs; the draw itself is always done in float64."""
from __future__ import annotations

import torch

from tests import pos_oracle as po


def draw(logp, u, temperature):
    """Row-wise oracle.xgate_oracle.sample_token: logp (M,C), u (M,) -> (M,) int64.  w = exp((logp - max logp) / temperature) in
    float64, the first index whose running sum exceeds u * total, clamped to C - 1.  (The row maximum is taken out first, as the
    header states the rule: the same distribution, and a low temperature then cannot underflow every weight.)"""
    lp = logp.double()
    w = torch.exp((lp - lp.max(1, keepdim=True).values) / temperature)
    cdf = torch.cumsum(w, 1)
    target = (u.double() * cdf[:, -1]).unsqueeze(1)
    return torch.searchsorted(cdf, target, side="right").squeeze(1).clamp(max=logp.shape[1] - 1)


@torch.no_grad()
def sample_templates(P, run, fr, fo, fm, uniforms, L, temperature=1.0):
    """uniforms (B,S,L).  Returns a dict: templates (B,S,L) int64, tag_logp (B,S,L), states (B,S,L+1,R), masks (B,S,L+1),
    pos_feats (B*S,R), n, and logps: the L per-step (B*S,C) log-probabilities each draw was made from (for the edge rule of
    tests.util.assert_sampled_tokens_match).  All L + 1 steps run; a finished row holds its state (mask 0)."""
    uniforms = torch.as_tensor(uniforms).to(fr.device)
    B, S, Lu = uniforms.shape
    assert Lu == L
    V, q, h, c = po._prologue(P, run, fr, fo, fm)
    V, q, h, c = (t.repeat_interleave(S, 0) for t in (V, q, h, c))
    M = B * S
    um = uniforms.reshape(M, L)
    unf = torch.ones(M, dtype=fr.dtype, device=fr.device)
    states, masks, tlp, toks, logps = [], [], [], [], []
    logp = None
    for t in range(L + 1):
        if t == 0:
            it = torch.zeros(M, dtype=torch.int64, device=fr.device)
        else:
            it = draw(logp, um[:, t - 1], temperature)
            logps.append(logp)
            # counted while the row was unfinished BEFORE this tag: up to and including its first 0
            tlp.append(logp.gather(1, it.unsqueeze(1)).squeeze(1) * unf)
            unf = unf * (it > 0).to(fr.dtype)
            it = it * unf.long()
            toks.append(it)
        h, c, logp = po.step(P, V, q, it, unf.unsqueeze(1), h, c)
        states.append(h)
        masks.append(unf)
    tm = torch.stack(toks, 1)
    lead = (tm > 0).to(torch.int64).cumprod(1).sum(1)
    R = h.shape[1]
    return dict(templates=tm.reshape(B, S, L), tag_logp=torch.stack(tlp, 1).reshape(B, S, L),
                states=torch.stack(states, 1).reshape(B, S, L + 1, R), masks=torch.stack(masks, 1).reshape(B, S, L + 1),
                pos_feats=h, n=min(L, int(lead.max())), logps=logps)
