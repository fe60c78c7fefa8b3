#!/usr/bin/env python3
"""Generate the POS generator's TRAINING fixtures tests/golden/pos_train_*.npz from the REFERENCE itself.

Runs the reference's pos_src/SAModel.py in train mode on CPU with the shims of tools/gen_pos_golden.py, as its own process.  The three
nn.Dropout modules of the reference get the hash masks of oracle.paramgen.keep_mask in place of their random ones, in call order:
two_fc_encoder.drop_out on rgb (site 0) then on opfl (site 1), fusion.late_fusion[2] (site 4), lstmcore.lstmcell.dropout at step t
(site 6, step t) -- so the dropout placement is pinned to the reference, not only to tests/pos_train_oracle.py.  Records, per case of
pos_train_oracle.TRAIN_CASES: the loss, every parameter's gradient (all elements up to 4096, else a name-seeded sample + max-abs +
norm), the BatchNorm batch statistics and the updated running statistics; and a three-iteration trajectory under the reference's
torch.optim.Adam + myutils.clip_gradient at p = 0 (losses and the parameters after each step).

    python tools/gen_pos_train_golden.py        # writes tests/golden/pos_train_*.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import paramgen as pg  # noqa: E402
from tests import pos_oracle as po  # noqa: E402
from tests import pos_train_oracle as pto  # noqa: E402
import gen_pos_golden as gpg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FULL_MAX = 4096


def hash_dropouts(model, p, seed):
    """Replace the forward of the reference's three nn.Dropout modules by the hash masks, in call order."""
    calls = {"enc": 0, "cell": 0}

    def enc_drop(x):
        site = pto.SITE_EMB_RGB if calls["enc"] % 2 == 0 else pto.SITE_EMB_OPFL
        calls["enc"] += 1
        return x * pto.mask(seed, site, 0, tuple(x.shape), p)

    def fusion_drop(x):
        return x * pto.mask(seed, pto.SITE_FUSION, 0, tuple(x.shape), p)

    def cell_drop(x):
        t = calls["cell"]
        calls["cell"] += 1
        return x * pto.mask(seed, pto.SITE_CELL, t, tuple(x.shape), p)

    model.two_fc_encoder.drop_out.forward = enc_drop
    model.two_fc_encoder.fusion.late_fusion[2].forward = fusion_drop
    model.lstmcore.lstmcell.dropout.forward = cell_drop
    return calls


def store_grads(g, named):
    for n, prm in named:
        v = (prm.grad if prm.grad is not None else torch.zeros_like(prm)).detach().numpy().astype(np.float32)
        if v.size <= FULL_MAX:
            g["g/" + n] = v
        else:
            idx = pto.sample_index(n, v.size)
            g["gi/" + n] = idx
            g["gs/" + n] = v.reshape(-1)[idx]
            g["gmax/" + n] = np.float32(np.abs(v).max())
            g["gnorm/" + n] = np.float64(np.linalg.norm(v.astype(np.float64)))


def bn_hooks(model, g):
    def hook(name):
        def f(mod, inp, out):
            z = inp[0].detach()
            g["bn_mean/" + name] = z.mean(0).numpy()
            g["bn_var/" + name] = z.var(0, unbiased=False).numpy()
        return f
    e = model.two_fc_encoder
    return [e.visual_emb_rgb[1].register_forward_hook(hook("rgb")), e.visual_emb_opfl[1].register_forward_hook(hook("opfl"))]


def inputs(x):
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    return fr, fo, fm, cap_r, new_mask, torch.from_numpy(x["class_mask"])


def loss_of(ref, out, cap_r, new_mask, cm):
    if out.shape[1] == cap_r.shape[1]:
        return ref.ClassiferCriterion()(out, cap_r, new_mask, cm)
    return po.criterion(out, cap_r, new_mask, cm)          # (the reference's criterion needs the full width)


def gen_case(ref, name):
    cfg, kw, p, seed = pto.TRAIN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, **kw)
    with gpg.quiet():
        model, _, _ = gpg.build_ref(ref, d, P, run, p_drop=p)
    model.train()
    calls = hash_dropouts(model, p, seed)
    g = {}
    hooks = bn_hooks(model, g)
    fr, fo, fm, cap_r, new_mask, cm = inputs(x)
    with gpg.quiet():
        out = model(fr, fo, fm, None, None, cap_r, new_mask)
        loss = loss_of(ref, out, cap_r, new_mask, cm)
        loss.backward()
    for h in hooks:
        h.remove()
    assert calls["enc"] == 2 and calls["cell"] == out.shape[1], calls
    g["loss"] = np.float64(loss.item())
    g["tf_T"] = np.int64(out.shape[1])
    store_grads(g, list(model.named_parameters()))
    sd = model.state_dict()
    for m in ("rgb", "opfl"):
        for b in ("running_mean", "running_var"):
            g["run/%s/%s" % (m, b)] = sd["two_fc_encoder.visual_emb_%s.1.%s" % (m, b)].numpy().copy()
    np.savez_compressed(os.path.join(GOLD, "pos_train_%s.npz" % name), **g)
    print("pos_train_%s: loss %.6f  T' %d/%d" % (name, g["loss"], out.shape[1], cap_r.shape[1]))


def gen_traj(ref):
    cfg, kw = pto.TRAJ_CASE
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, **kw)
    with gpg.quiet():
        model, _, _ = gpg.build_ref(ref, d, P, run, p_drop=0.0)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=pto.TRAJ_LR)
    fr, fo, fm, cap_r, new_mask, cm = inputs(x)
    g = {}
    losses = []
    for it in range(pto.TRAJ_STEPS):
        opt.zero_grad()
        with gpg.quiet():
            out = model(fr, fo, fm, None, None, cap_r, new_mask)
            loss = loss_of(ref, out, cap_r, new_mask, cm)
            loss.backward()
        for group in opt.param_groups:                      # myutils.clip_gradient
            for prm in group["params"]:
                prm.grad.data.clamp_(-pto.TRAJ_CLIP, pto.TRAJ_CLIP)
        opt.step()
        losses.append(loss.item())
        for n, prm in model.named_parameters():
            g["p%d/%s" % (it, n)] = prm.detach().numpy().copy()
    g["losses"] = np.array(losses, np.float64)
    sd = model.state_dict()
    for m in ("rgb", "opfl"):
        for b in ("running_mean", "running_var"):
            g["run/%s/%s" % (m, b)] = sd["two_fc_encoder.visual_emb_%s.1.%s" % (m, b)].numpy().copy()
    np.savez_compressed(os.path.join(GOLD, "pos_train_traj.npz"), **g)
    print("pos_train_traj: losses %s" % losses)


def main():
    if not os.path.isdir(gpg.REF):
        print("reference not present; nothing to do")
        return 0
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    torch.manual_seed(0)
    ref = gpg.import_reference()
    for name in pto.TRAIN_CASES:
        gen_case(ref, name)
    gen_traj(ref)
    return 0


if __name__ == "__main__":
    sys.exit(main())
