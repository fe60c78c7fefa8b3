"""Shared helpers for the parity tests (test infrastructure)."""
import os
import re

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

CFG = {
    "c1": dict(B=8, K=26, R=512, A=1536, E=468, V=20000, C=14, L=20, F1=1536, F2=1024, H=128),
    "tiny": dict(B=5, K=7, R=24, A=40, E=18, V=61, C=5, L=6, F1=20, F2=12, H=128),
    "c5": dict(B=4, K=40, R=1024, A=1536, E=468, V=20000, C=14, L=6, F1=1536, F2=1024, H=128),
    # nothing aligned: R not a multiple of 8 (generic cell path, no skinny kernel), odd E / A / V, B = 3
    "odd": dict(B=3, K=3, R=20, A=37, E=10, V=37, C=3, L=4, F1=9, F2=7, H=128),
    # degenerate extents: one video, one frame, one word
    "one": dict(B=1, K=1, R=8, A=8, E=4, V=5, C=2, L=1, F1=4, F2=4, H=128),
    # mid-size, everything 16-byte aligned: exercises the vector-load GEMM paths quickly
    "mid": dict(B=12, K=9, R=64, A=96, E=36, V=500, C=14, L=7, F1=48, F2=40, H=128),
}
WEIGHT_CLASS = 0.5
# greedy_c1_eos.npz (tools/gen_golden.py:EOS_CASE): embed x15, row 0 of logit.weight x4, inputs of seed 2
EOS_CASE = dict(embed_gain=15.0, eos_row_gain=4.0, input_seed=2)


def eos_params(d):
    """Weights of the natural-EOS greedy golden (same scaling as tools/gen_golden.py:eos_params)."""
    P = pg.make_params(d)
    P["embed.weight"] = P["embed.weight"] * np.float32(EOS_CASE["embed_gain"])
    P["logit.weight"] = P["logit.weight"].copy()
    P["logit.weight"][0] *= np.float32(EOS_CASE["eos_row_gain"])
    return P


def load_golden(name):
    return np.load(os.path.join(GOLD, name))


def header_symbols():
    """Function names declared in include/xgate.h."""
    txt = open(os.path.join(ROOT, "include", "xgate.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(xg_[a-z_0-9]+)\s*\(", txt)))


def make_model(d, P=None, device="cuda", p_drop=0.0, train=True, precision="fp32"):
    from controllable_xgating_amd import SAModel, make_opt
    model = SAModel(make_opt(d, drop_prob_lm=p_drop, precision=precision))
    if P is None:
        P = pg.make_params(d)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=False)
    assert not missing.unexpected_keys
    model = model.to(device)
    model.train(train)
    return model


def to_dev(x, device="cuda"):
    return {k: torch.from_numpy(v).to(device) for k, v in x.items()}


def oracle_grads(P):
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for k, v in P.items()}


# parameters whose TRUE gradient is exactly zero (a Linear bias in front of train-mode BatchNorm; a2w.bias, which cancels in
# the softmax): what is left is round-off of cancelling terms, of no fixed size
ZERO_GRAD_PARAMS = ("two_spatial_encoder.visual_emb_rgb.0.bias", "two_spatial_encoder.visual_emb_opfl.0.bias", "lstmcore.a2w.bias")


# ReLU sites of the oracle (oracle/xgate_oracle.py: relu_trace) -> the Linear in front of the ReLU, and the BatchNorm between
# them for the encoder embeddings.  A flipped ReLU derivative at element (.., j) of a site moves only what it feeds: row j of that
# Linear's weight gradient, element j of its bias (and of the BatchNorm's weight and bias), and for the decoder's POS gate the
# embedding rows of the tokens fed at the flipped row.
FLIP_SITES = {
    "enc.rgb": (xo.ENC + "visual_emb_rgb.0", xo.ENC + "visual_emb_rgb.1"),
    "enc.opfl": (xo.ENC + "visual_emb_opfl.0", xo.ENC + "visual_emb_opfl.1"),
    "gate_rgb": (xo.ENC + "gate_rgb.gate.0", None),
    "gate_opfl": (xo.ENC + "gate_opfl.gate.0", None),
    "fusion": (xo.ENC + "fusion.late_fusion.0", None),
    "pos_gate": ("lstmcore.gate.gate.0", None),
    "classifer": ("classifer.0", None),
}
# flip candidate: |float64 pre-activation| <= FLIP_C * (largest |fp32 - fp64| pre-activation difference at that site).  The HIP
# products sum in other orders than the fp32 oracle (MFMA chains, split-K), so their round-off is of the fp32 oracle's size but not
# the same; 8 leaves room for that (measured: see flip_exemptions).  FLIP_SHARE_MAX bounds the candidates per site so that the
# exemption cannot grow silently.
FLIP_C = 8.0
FLIP_SHARE_MAX = 1e-3


def run_oracle(Pn, xn, fn, dtype=torch.float32, grad=True):
    """Run ``fn(P, xi, relu_trace) -> (loss, extra)`` on the oracle with parameters and float inputs cast to `dtype` and torch's
    default dtype set to it (tools/r6/drop_diag.py), then backward.  Returns (loss float, extra, grads {name: float64 ndarray} or
    None, relu_trace)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(grad) for k, v in Pn.items()}
        xi = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in xo.to_torch_inputs(xn).items()}
        trace = []
        with torch.set_grad_enabled(grad):
            loss, extra = fn(P, xi, trace)
            if grad:
                loss.backward()
    finally:
        torch.set_default_dtype(old)
    grads = None
    if grad:
        grads = {k: (v.grad.double().numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()}
    return loss.item(), extra, grads, trace


def flip_exemptions(trace64, trace32, shapes, c=FLIP_C, share_max=FLIP_SHARE_MAX, counts=None):
    """Elements of the gradients that a flipped ReLU derivative may move: {param name: bool mask}.  `trace64` / `trace32`: the
    relu_trace of the same oracle call in float64 and float32 (same inputs, masks and seed); `shapes`: {param name: shape}.
    A candidate is an element whose |float64 pre-activation| is at most c times the largest |fp32 - fp64| difference at its site
    (all steps / frames of a site together); each exempts exactly what it feeds (FLIP_SITES).  Asserts that no site has more than
    `share_max` of its elements as candidates.  `counts`: optional dict filled with {site: (candidates, elements)}."""
    assert [t[0] for t in trace64] == [t[0] for t in trace32]
    by_site = {}
    for (site, a, tok), (_, b, _) in zip(trace64, trace32):
        by_site.setdefault(site, []).append((a.double(), b.double(), tok))
    ex = {}

    def mark(name, idx, rows=True):
        m = ex.setdefault(name, np.zeros(shapes[name], bool))
        if rows:
            m[idx] = True
        else:
            m[idx, ...] = True

    for site, items in by_site.items():
        lin, bn = FLIP_SITES[site]
        dmax = max(float((b - a).abs().max()) for a, b, _ in items)
        n = tot = 0
        for a, _, tok in items:
            cand = (a.abs() <= c * dmax).reshape(-1, a.shape[-1]).numpy()
            n += int(cand.sum())
            tot += cand.size
            cols = np.flatnonzero(cand.any(0))
            if cols.size == 0:
                continue
            mark(lin + ".weight", cols)
            mark(lin + ".bias", cols)
            if bn is not None:
                mark(bn + ".weight", cols)
                mark(bn + ".bias", cols)
            if site == "pos_gate":
                assert tok is not None
                mark("embed.weight", np.unique(tok.numpy()[np.flatnonzero(cand.any(1))]))
        assert n <= share_max * tot, (site, n, tot)
        if counts is not None:
            counts[site] = (n, tot)
    return ex


# parameters whose TRUE gradient is exactly zero (a Linear bias in front of train-mode BatchNorm; a2w.bias, which cancels in
# the softmax): what is left is round-off of cancelling terms, of no fixed size
ZERO_GRAD_PARAMS = ("two_spatial_encoder.visual_emb_rgb.0.bias", "two_spatial_encoder.visual_emb_opfl.0.bias", "lstmcore.a2w.bias")


def grad_misses(grads, ref, rtol=2e-3, atol=2e-6, skip=(), cos_min=1 - 1e-5, rtol_elem=None, report=None, exempt=None, elem_share=0.1):
    """Three bounds per parameter (round 5: the max-norm bound alone lets a defect confined to a gradient's small entries through):
    (1) max |g - r| <= atol + rtol * max |r|; (2) direction: cosine(g, r) >= cos_min; (3) element-wise: |g_i - r_i| <=
    atol + rtol |r_i| + (rtol / 10) max |r| -- the share of the bound that does not scale with the element itself is a tenth
    of (1)'s (`elem_share`; 1.0 leaves (3) to (1): for errors that do not scale with the element they land on -- tests/bf16_oracle.py).
    `grads` / `ref`: {name: ndarray}.  `exempt`: optional {name: bool mask} (flip_exemptions) -- the masked elements are
    left out of all three bounds, every other element keeps them; max |r| is still taken over the whole parameter.
    Parameters whose true gradient is exactly zero (ZERO_GRAD_PARAMS) only make sense under (1) with their own scale and are
    passed in `skip` by the callers.  `report`: optional dict filled with (max error / scale, cosine, worst element-wise
    error / bound, exempted elements) per parameter.  Returns the list of misses."""
    bad = []
    rt_e = rtol if rtol_elem is None else rtol_elem
    for name, g in grads.items():
        if name in skip:
            continue
        r = ref[name]
        scale = np.abs(r).max()
        keep = None if exempt is None or name not in exempt else ~exempt[name]
        if keep is not None:
            g, r = g[keep], r[keep]
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        err = np.abs(g - r).max() if g.size else 0.0
        if not err <= atol + rtol * scale:
            bad.append((name, "max", float(err), float(scale)))
        gd, rd = g.ravel(), r.ravel()
        nr, ng = np.linalg.norm(rd), np.linalg.norm(gd)
        cos = float(gd @ rd / (nr * ng)) if nr > 0 and ng > 0 else (1.0 if nr == ng else 0.0)
        # (a gradient whose norm is itself at round-off level has no direction to speak of)
        if nr > 50 * atol * np.sqrt(rd.size) and not cos >= cos_min:
            bad.append((name, "cosine", cos, float(scale)))
        ratio = np.abs(g - r) / (atol + rt_e * np.abs(r) + elem_share * rtol * scale)
        if g.size and not ratio.max() <= 1:
            i = int(np.argmax(ratio))
            bad.append((name, "element", float(np.abs(g - r).ravel()[i]), float(np.abs(r).ravel()[i]), float(scale)))
        if report is not None:
            report[name] = (float(err / max(scale, 1e-30)), cos, float(ratio.max()) if g.size else 0.0,
                            0 if keep is None else int((~keep).sum()))
    return bad


def model_grads(model):
    return {name: (p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
            for name, p in model.named_parameters()}


def assert_grads_close(model, ref, rtol=2e-3, atol=2e-6, skip=(), cos_min=1 - 1e-5, rtol_elem=None, report=None, exempt=None):
    """grad_misses over the model's parameter gradients; fails on any miss."""
    bad = grad_misses(model_grads(model), ref, rtol, atol, skip, cos_min, rtol_elem, report, exempt)
    assert not bad, bad


def oracle_f64_with_flips(Pn, xn, fn, counts=None):
    """The float64 oracle for a case with ReLU-flip exposure: ``fn`` (run_oracle's form) runs once in float64 with gradients and
    once in float32 for the pre-activations.  Returns (loss, extra, grads, exempt) -- compare a kernel's gradients with `grads`
    under `exempt` (grad_misses); `counts` as in flip_exemptions."""
    loss, extra, g64, t64 = run_oracle(Pn, xn, fn, torch.float64)
    _, _, _, t32 = run_oracle(Pn, xn, fn, torch.float32, grad=False)
    ex = flip_exemptions(t64, t32, {k: v.shape for k, v in Pn.items()}, counts=counts)
    return loss, extra, g64, ex


def _pad(a, n):
    return np.concatenate([a, np.zeros((a.shape[0], n - a.shape[1]), a.dtype)], 1)


def assert_sampled_tokens_match(s_h, s_o, logps_o, u, temperature=1.0, tol=3e-4):
    """Tokens a kernel drew from the uniforms `u` (L+1, B) vs the oracle's own draw `s_o` (xo.sample(mode='sample'), with its
    per-step log-probs `logps_o`): every row equal, except a row whose FIRST difference is a draw whose uniform lies within `tol`
    of an edge of the oracle's float64 CDF interval (of exp(logp / temperature)) -- where the log-probs' round-off may pick the
    neighbouring token; the rest of such a row follows other tokens and is not compared.  Returns the rows that differ."""
    s_h, s_o = np.asarray(s_h), np.asarray(s_o)
    n = max(s_h.shape[1], s_o.shape[1])
    s_h, s_o = _pad(s_h, n), _pad(s_o, n)
    rows = []
    for b in np.flatnonzero((s_h != s_o).any(1)):
        k = int(np.flatnonzero(s_h[b] != s_o[b])[0])
        assert k < len(logps_o), (b, k)
        cdf = np.cumsum(np.exp(logps_o[k][b].detach().double().numpy() / temperature))
        tok = int(s_o[b, k])
        lo, hi = (cdf[tok - 1] if tok > 0 else 0.0) / cdf[-1], cdf[tok] / cdf[-1]
        uu = float(u[k + 1, b])
        assert min(abs(uu - lo), abs(uu - hi)) <= tol, (b, k, int(s_h[b, k]), tok, lo, uu, hi)
        rows.append(int(b))
    return rows


def assert_greedy_tokens_match(g_h, g_o, logps_o, margin=1e-3):
    """Greedy tokens vs the oracle's greedy rollout: equal, except a row whose first difference is at a step where the oracle's
    top-2 log-prob margin is below `margin` (round-off may take either); the rest of such a row is not compared."""
    g_h, g_o = np.asarray(g_h), np.asarray(g_o)
    n = max(g_h.shape[1], g_o.shape[1])
    g_h, g_o = _pad(g_h, n), _pad(g_o, n)
    for b in np.flatnonzero((g_h != g_o).any(1)):
        k = int(np.flatnonzero(g_h[b] != g_o[b])[0])
        top2 = np.sort(logps_o[k][b].detach().double().numpy())[-2:]
        assert top2[1] - top2[0] < margin, (b, k, int(g_h[b, k]), int(g_o[b, k]), top2[1] - top2[0])


def oracle_rollouts(d, Pn, xn, u, seed, p, temperature=1.0, train=True, policy=None, dtype=torch.float32):
    """The oracle's own sampled (from `u`) and greedy rollouts under dropout seed `seed`: ((seq, logps), (seq, logps)).
    `policy`: the oracle's bf16 rounding policy (tests/bf16_oracle.py); `dtype`: the arithmetic of the oracle."""
    if policy is not None or dtype != torch.float32:
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in Pn.items()}
            xi = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in xo.to_torch_inputs(xn).items()}
            args = (P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L)
            with torch.no_grad():
                s, _, lps = xo.sample(*args, mode="sample", uniforms=u, temperature=temperature, train=train, p=p, seed=seed,
                                      running=xo.new_running(d), return_logp=True, policy=policy)
                g, _, lpg = xo.sample(*args, mode="greedy", train=train, p=p, seed=seed, running=xo.new_running(d), return_logp=True,
                                      policy=policy)
        finally:
            torch.set_default_dtype(old)
        return (s.numpy(), lps), (g.numpy(), lpg)
    P = xo.to_torch_params(Pn)
    xi = xo.to_torch_inputs(xn)
    args = (P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L)
    with torch.no_grad():
        s, _, lps = xo.sample(*args, mode="sample", uniforms=u, temperature=temperature, train=train, p=p, seed=seed,
                              running=xo.new_running(d), return_logp=True)
        g, _, lpg = xo.sample(*args, mode="greedy", train=train, p=p, seed=seed, running=xo.new_running(d), return_logp=True)
    return (s.numpy(), lps), (g.numpy(), lpg)


def check_sampled_rollout(model, d, Pn, xn, u, reward, seq, slp, loss, seed, p, temperature=1.0, lp_tol=3e-4, loss_tol=1e-4,
                          grad_kw=None, bn_updates=1, counts=None, report=None, policy=None):
    """A kernel's sampled rollout (`seq`, `slp`: trimmed; `loss`: its RewardCriterion with `reward`, already backpropagated into
    `model`) vs
    the oracle under dropout seed `seed`: tokens up to CDF-boundary draws (assert_sampled_tokens_match); then the oracle replays
    the kernel's tokens in float64 (oracle_f64_with_flips) -- seqLogprobs (the UNTEMPERED log-probs: SAModel.py:189-195) within
    `lp_tol`, the loss within `loss_tol`, every gradient with grad_misses, and the BatchNorm running statistics after
    `bn_updates` train-mode updates.  `policy`: the oracle's bf16 rounding policy -- the draw (in float64) and the replay then
    round where the kernels of precision="bf16" round (tests/bf16_oracle.py)."""
    (s_o, lps), _ = oracle_rollouts(d, Pn, xn, u, seed, p, temperature, policy=policy, dtype=torch.float32 if policy is None else torch.float64)
    seq, slp = seq.cpu().numpy(), slp.detach().cpu().numpy()
    assert_sampled_tokens_match(seq, s_o, lps, u, temperature)
    n = seq.shape[1]
    forced = torch.from_numpy(seq)

    def fn(P, xi, tr):
        running = xo.new_running(d)
        so, lp = xo.sample(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L, mode="replay",
                           forced=forced, train=True, p=p, seed=seed, running=running, relu_trace=tr, policy=policy)
        for _ in range(bn_updates - 1):
            xo.encoder_fwd(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], True, p, seed, running)
        return xo.reward_criterion(lp, so, torch.from_numpy(reward[:, :n]).to(lp.dtype)), (lp.detach().numpy(), running)

    loss_o, (lp_o, running), g64, ex = oracle_f64_with_flips(Pn, xn, fn, counts)
    m = np.concatenate([np.ones((d.B, 1), bool), seq[:, :-1] > 0], 1)
    np.testing.assert_allclose(slp[m], lp_o[m], atol=lp_tol)
    assert abs(loss - loss_o) < loss_tol, (loss, loss_o)
    bad = grad_misses(model_grads(model), g64, skip=ZERO_GRAD_PARAMS, exempt=ex, report=report, **(grad_kw or {}))
    assert not bad, bad
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), running[pre + "running_mean"].numpy(), atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), running[pre + "running_var"].numpy(), atol=1e-5)
