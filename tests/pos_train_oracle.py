"""TEST INFRASTRUCTURE ONLY -- a CPU torch restatement of the POS sequence generator in TRAIN mode (reference pos_src/SAModel.py,
pos_src/sub_modules.py, starttrain_trainpos.py:138-152), with autograd for the gradients.

What train mode changes against tests/pos_oracle.py: BatchNorm1d normalises with the batch statistics over all B K rows (masked
frames included) and updates the running statistics (momentum 0.1, unbiased variance); the dropouts are hash masks
(oracle.paramgen.keep_mask) at the captioner's site numbers -- 0 the rgb embedding and 1 the opfl embedding (sub_modules.py:204,209,
after BN + ReLU, before the frame mask), 4 the fusion's ReLU output (:63-66), 6 the decoder cell's h at step t AFTER the mask hold
(:884-887: the dropped h is both the state and the head's input).  tests/golden/pos_train_*.npz pin it to the reference itself
(tools/gen_pos_train_golden.py).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import paramgen as pg  # noqa: E402
from tests import pos_oracle as po  # noqa: E402

SITE_EMB_RGB, SITE_EMB_OPFL, SITE_FUSION, SITE_CELL = 0, 1, 4, 6
BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def mask(seed, site, step, shape, p, dtype=torch.float32, device="cpu", cache=None):
    """The hash-dropout multiplier as a tensor on `device`.  `cache`: optional dict that keeps the masks once built (the eager
    baseline of tools/pos_train_bench.py builds them outside its timed loop, so that it times the model and not the host hash)."""
    key = (seed, site, step, tuple(shape), p, dtype, str(device))
    if cache is not None and key in cache:
        return cache[key]
    m = torch.from_numpy(pg.keep_mask(seed, site, step, shape, p)).to(device=device, dtype=dtype)
    if cache is not None:
        cache[key] = m
    return m


def _lin(x, P, name):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def encoder(P, run, fr, fo, fm, p, seed, stats=None, train=True, cache=None):
    """V (B,K,R); `run` (running statistics) is updated in place when train; `stats` receives the batch mean / biased var."""
    B, K = fr.shape[:2]
    dt = fr.dtype
    outs = []
    for m, x, site in (("rgb", fr, SITE_EMB_RGB), ("opfl", fo, SITE_EMB_OPFL)):
        pre = f"two_fc_encoder.visual_emb_{m}."
        z = _lin(x.reshape(B * K, -1), P, pre + "0")
        if train:
            mean = z.mean(0)
            var = z.var(0, unbiased=False)
            zn = (z - mean) / torch.sqrt(var + BN_EPS) * P[pre + "1.weight"] + P[pre + "1.bias"]
            n = z.shape[0]
            with torch.no_grad():
                rm, rv = run[pre + "1.running_mean"], run[pre + "1.running_var"]
                rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.detach().to(rm.dtype))
                rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * (var.detach() * n / max(n - 1, 1)).to(rv.dtype))
            if stats is not None:
                stats[m + "_mean"], stats[m + "_var"] = mean.detach(), var.detach()
        else:
            zn = F.batch_norm(z, run[pre + "1.running_mean"].to(dt), run[pre + "1.running_var"].to(dt), P[pre + "1.weight"],
                              P[pre + "1.bias"], False, 0.0, BN_EPS)
        emb = torch.relu(zn).reshape(B, K, -1)
        emb = emb * mask(seed, site, 0, tuple(emb.shape), p, dt, fr.device, cache) * fm.unsqueeze(-1)
        c = f"two_fc_encoder.lstmcell_{m}."
        R = emb.shape[-1]
        h = emb.new_zeros(B, R)
        cs = emb.new_zeros(B, R)
        hs = []
        for k in range(K):
            g = F.linear(emb[:, k], P[c + "weight_ih"], P[c + "bias_ih"]) + F.linear(h, P[c + "weight_hh"], P[c + "bias_hh"])
            i, f, gg, o = g.chunk(4, 1)
            cs = torch.sigmoid(f) * cs + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(cs)
            mk = fm[:, k:k + 1]
            h, cs = h * mk, cs * mk
            hs.append(h)
        outs.append(torch.stack(hs, 1))
    V = torch.relu(_lin(torch.cat(outs, -1), P, "two_fc_encoder.fusion.late_fusion.0"))
    return V * mask(seed, SITE_FUSION, 0, tuple(V.shape), p, dt, fr.device, cache)


def step(P, V, q, tok, m, h, c, keep):
    e = F.linear(torch.tanh(_lin(h, P, "lstmcore.h2a").unsqueeze(1) + q), P["lstmcore.a2w.weight"], P["lstmcore.a2w.bias"])
    alpha = torch.softmax(e, dim=1)
    af = (alpha * V).sum(1)
    s = (_lin(P["embed.weight"][tok], P, "lstmcore.lstmcell.i2h") + _lin(af, P, "lstmcore.lstmcell.a2h") +
         _lin(h, P, "lstmcore.lstmcell.h2h"))
    i, f, o, g = s.chunk(4, 1)
    cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    cn = cn * m + c * (1 - m)
    hn = torch.sigmoid(o) * torch.tanh(cn)
    hn = (hn * m + h * (1 - m)) * keep
    return hn, cn, F.log_softmax(_lin(hn, P, "logit"), dim=1)


def forward_train(P, run, fr, fo, fm, cap_r, new_mask, p=0.0, seed=0, stats=None, train=True, cache=None):
    """(B, T', C) train-mode log-probabilities (differentiable wrt P); the loop stops at the first i >= 1 whose category column is
    all zero."""
    V = encoder(P, run, fr, fo, fm, p, seed, stats, train, cache)
    with torch.no_grad():
        mean = (V.sum(1) / fm.sum(1, keepdim=True)).detach()           # init_hidden: detached (SAModel.py:54-60)
    h, c = _lin(mean, P, "img_embed_h_1"), _lin(mean, P, "img_embed_c_1")
    q = _lin(V, P, "lstmcore.v2a")
    B, R = h.shape
    outs = []
    for i in range(cap_r.shape[1]):
        if i >= 1 and int(cap_r[:, i].sum()) == 0:
            break
        keep = mask(seed, SITE_CELL, i, (B, R), p, fr.dtype, fr.device, cache)
        h, c, lp = step(P, V, q, cap_r[:, i], new_mask[:, i:i + 1].to(fr.dtype), h, c, keep)
        outs.append(lp)
    return torch.stack(outs, 1)


def criterion(logp, target, mask_, class_mask=None):
    return po.criterion(logp, target, mask_, class_mask)


def params(P, dtype=torch.float32, requires_grad=True, device="cpu"):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, device=device, requires_grad=requires_grad) for k, v in P.items()}


def running(run, dtype=torch.float32, device="cpu"):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, device=device) for k, v in run.items()}


def loss_and_grads(d, P, run, x, p=0.0, seed=0, dtype=torch.float32, device="cpu"):
    """One train-mode forward + ClassiferCriterion + backward: (loss, {name: grad}, {stat: value}, updated running statistics,
    logp), as numpy.  Parameters without a gradient path get zeros.  `device`: where torch runs it (a GPU for the eager baseline
    or a fast float64 reference)."""
    Pt, rt = params(P, dtype, device=device), running(run, dtype, device=device)
    fr, fo, fm = (torch.from_numpy(x[k]).to(device=device, dtype=dtype) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    cap_r, new_mask = cap_r.to(device), new_mask.to(device)
    cm = torch.from_numpy(x["class_mask"]).to(device=device, dtype=dtype)
    stats = {}
    out = forward_train(Pt, rt, fr, fo, fm, cap_r, new_mask.to(dtype), p, seed, stats)
    loss = criterion(out, cap_r, new_mask.to(dtype), cm)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().cpu().numpy() for k, v in Pt.items()}
    return (loss.item(), grads, {k: v.cpu().numpy() for k, v in stats.items()}, {k: v.cpu().numpy() for k, v in rt.items()},
            out.detach().cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------------------------
# fixtures: tests/golden/pos_train_<name>.npz (tools/gen_pos_train_golden.py)
# name -> (POS_CFG key, make_inputs kwargs, drop_p, dropout seed)
TRAIN_CASES = {
    "tiny": ("tiny", dict(seed=0), 0.0, 0),
    "ragged": ("mid", dict(seed=2, ragged=True), 0.0, 0),
    "c1": ("c1", dict(seed=1), 0.0, 0),
    "drop": ("mid", dict(seed=3, ragged=True), 0.5, 1234),
    "tfzero": ("tiny", dict(seed=4, ragged=True, max_words=3), 0.0, 0),
}
TRAJ_CASE = ("tiny", dict(seed=5, ragged=True))      # three Adam iterations at p = 0
TRAJ_LR, TRAJ_CLIP, TRAJ_STEPS = 4e-3, 0.1, 3
SAMPLE_PER_PARAM = 64                                # c1: stored elements per parameter (name-seeded positions)


def sample_index(name, numel, k=SAMPLE_PER_PARAM):
    """Fixed, name-seeded flat positions of a parameter's stored gradient sample (all of them when it is small)."""
    if numel <= k:
        return np.arange(numel)
    u = pg.uniform("pos_train/sample/" + name, (k,), 0)
    return np.unique((u * numel).astype(np.int64))


def clip_adam(Pt, grads, state, step, lr=TRAJ_LR, clip=TRAJ_CLIP, b1=0.9, b2=0.999, eps=1e-8):
    """myutils.clip_gradient (clamp to +-clip) + torch.optim.Adam, element for element, in float64."""
    out = {}
    for k, v in Pt.items():
        g = np.clip(grads[k].astype(np.float64), -clip, clip)
        m, s = state.setdefault(k, (np.zeros_like(g), np.zeros_like(g)))
        m = b1 * m + (1 - b1) * g
        s = b2 * s + (1 - b2) * g * g
        state[k] = (m, s)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        out[k] = (np.asarray(v, np.float64) - lr / bc1 * m / (np.sqrt(s) / np.sqrt(bc2) + eps)).astype(np.float32)
    return out


# parameters whose true gradient is zero: the softmax over frames is shift-invariant (a2w.bias) and train-mode BatchNorm cancels the
# bias of the Linear in front of it; what an implementation computes there is round-off, compared with an absolute bound only
ZERO_GRAD = ("lstmcore.a2w.bias", "two_fc_encoder.visual_emb_rgb.0.bias", "two_fc_encoder.visual_emb_opfl.0.bias")


def traj_misses(P, P0, g, it, lr=TRAJ_LR):
    """Parameters after iteration `it` against the trajectory fixture.  Adam normalises the gradient: an element whose gradient
    is at round-off level may step differently, so the value is compared at 3.1 lr per step taken and the displacement at 10 % of
    lr for all but 2 % of the elements.  ZERO_GRAD parameters are skipped."""
    bad = []
    for n, v in P.items():
        if n in ZERO_GRAD:
            continue
        r = g["p%d/%s" % (it, n)]
        v = np.asarray(v, np.float64)
        err = np.abs(v - r).max()
        if err > 3.1 * lr * (it + 1):
            bad.append((n, "value", float(err)))
        disp_err = np.abs((v - P0[n]) - (r - P0[n]))
        if (disp_err > 0.1 * lr).mean() > 0.02:
            bad.append((n, "displacement", float((disp_err > 0.1 * lr).mean())))
    return bad


def golden_grad_misses(grads, g, rtol=2e-3, atol=2e-6, zero_atol=1e-6):
    """grads {name: full array} against a fixture's full / sampled gradients; returns the misses."""
    bad = []
    for n, v in grads.items():
        if n in ZERO_GRAD:
            ref = g["g/" + n] if "g/" + n in g else g["gs/" + n]
            if np.abs(v).max() > zero_atol or np.abs(ref).max() > zero_atol:
                bad.append((n, "zero", float(np.abs(v).max()), float(np.abs(ref).max())))
            continue
        if "g/" + n in g:
            r, h = g["g/" + n].reshape(-1), v.reshape(-1)
            scale = np.abs(r).max()
        else:
            idx = g["gi/" + n]
            r, h = g["gs/" + n], v.reshape(-1)[idx]
            scale = float(g["gmax/" + n])
            nrm = np.linalg.norm(v.astype(np.float64))
            if abs(nrm - float(g["gnorm/" + n])) > rtol * float(g["gnorm/" + n]) + atol:
                bad.append((n, "norm", nrm, float(g["gnorm/" + n])))
            if abs(np.abs(v).max() - scale) > rtol * scale + atol:
                bad.append((n, "maxabs", float(np.abs(v).max()), scale))
        err = np.abs(h.astype(np.float64) - r).max()
        if err > atol + rtol * scale:
            bad.append((n, "max", float(err), float(scale)))
        elem = np.abs(h.astype(np.float64) - r) > atol + rtol * np.abs(r) + rtol / 10 * scale
        if elem.any():
            bad.append((n, "elem", int(elem.sum()), float(scale)))
    return bad
