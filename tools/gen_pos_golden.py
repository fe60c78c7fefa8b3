#!/usr/bin/env python3
"""Generate the POS generator's golden fixtures tests/golden/pos_*.npz from the REFERENCE itself.

Runs only where the reference tree exists: imports pos_src/SAModel.py on CPU with the same three shims as tools/gen_golden.py
(a stub h5py module, a no-op .cuda(), the `narrow(dimension=)` keyword), fills it with the seeded weights of tests/pos_oracle.py and
records outputs only (inputs are regenerated from seeds).  Run it as its own process: the reference's caption_src and pos_src both
have modules named SAModel and sub_modules.

    python tools/gen_pos_golden.py        # writes tests/golden/pos_*.npz
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pos_oracle as po  # noqa: E402

REF = "/root/reference/pos_src"
GOLD = os.path.join(ROOT, "tests", "golden")

# name -> (dims, input kwargs, EOS_CASE weights); the same table drives tests/test_gpu_pos.py
CASES = po.GOLDEN_CASES
STATE_COLS = 64          # states are stored for the first 64 hidden units (all of them below R = 64) + the last row in full


def import_reference():
    sys.modules["h5py"] = types.ModuleType("h5py")
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.cuda.manual_seed = lambda s: None
    _narrow = torch.Tensor.narrow

    def narrow(self, *a, **k):
        if "dimension" in k:
            k["dim"] = k.pop("dimension")
        return _narrow(self, *a, **k)

    torch.Tensor.narrow = narrow
    sys.path.insert(0, REF)
    sys.argv = ["x"]
    import SAModel as ref  # noqa
    return ref


def build_ref(ref, d, P, run, p_drop=0.0):
    opt = argparse.Namespace(seed=1024, category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, num_layers=1,
                             drop_prob_lm=p_drop, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2, att_size=d.A,
                             fusion_activity="ReLU")
    model = ref.SAModel(opt)
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    sd = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in po.make_state_dict(d, P, run).items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    return model, keys, shapes


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def gen_case(ref, name):
    cfg, kw, eos = CASES[name]
    kw = dict(kw)
    d = po.make_dims(**po.POS_CFG[cfg])
    P = po.make_params(d, eos=eos)
    run = po.make_running(d)
    x = po.make_inputs(d, **kw)
    model, keys, shapes = build_ref(ref, d, P, run)
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap = torch.from_numpy(x["cap_classes"])
    cmask = torch.from_numpy(x["class_mask"])
    cap_r, new_mask = po.prepare_targets(cap, cmask)
    seq_mask = torch.ones_like(new_mask)
    g = {"keys": np.array(keys), "shapes": np.array([",".join(map(str, s)) for s in shapes]), "cap_r": cap_r.numpy(),
         "new_mask": new_mask.numpy()}
    with quiet(), torch.no_grad():
        out = model(fr, fo, fm, None, None, cap_r, new_mask)
        g["tf_logp"] = out.numpy()
        g["tf_T"] = np.int64(out.shape[1])
        if out.shape[1] == cap_r.shape[1]:             # (the reference criterion needs the full width)
            g["loss"] = np.float64(ref.ClassiferCriterion()(out, cap_r, new_mask, cmask).item())
        logps = []
        hook = model.logit.register_forward_hook(lambda m, i, o: logps.append(torch.log_softmax(o, 1).numpy().copy()))
        seq, slp, states, masks = model.sample(fr, fo, fm, {"sample_max": 1, "beam_size": 1})
        hook.remove()
    s = seq.numpy()
    n = s.shape[1]
    lp = np.array(logps)[:n]                           # (n, B, C): the distribution of the choice at step t + 1
    top2 = -np.sort(-lp, axis=2)[:, :, :2]
    margin = top2[:, :, 0] - top2[:, :, 1]
    alive = np.ones_like(margin, bool)
    for b in range(d.B):
        z = np.flatnonzero(s[b] == 0)
        if z.size:
            alive[z[0] + 1:, b] = False
    g.update(seq=s, seqLogprobs=slp.numpy(), n=np.int64(n), masks=masks.numpy(), margin=margin, alive=alive,
             states=states.numpy()[:, :, :STATE_COLS].copy(), pos_feat=states.numpy()[:, -1].copy())
    np.savez_compressed(os.path.join(GOLD, "pos_%s.npz" % name), **g)
    lens = [int(np.flatnonzero(s[b] == 0)[0]) if (s[b] == 0).any() else -1 for b in range(d.B)]
    print("pos_%s: T' %d/%d  n %d  EOS at %s  min live margin %.2e  loss %s" % (
        name, out.shape[1], cap_r.shape[1], n, lens, margin[alive].min(), g.get("loss")))
    return g, d


def main():
    if not os.path.isdir(REF):
        print("reference not present; nothing to do")
        return 0
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    ref = import_reference()
    for name in CASES:
        g, d = gen_case(ref, name)
        if name == "eos":
            ended = (g["seq"] == 0).any(1)
            assert g["n"] < d.L and ended.any() and not ended.all(), "rows must finish at different steps, the batch before L"
            assert g["margin"][g["alive"]].min() >= 1e-3
        if name == "tfzero":
            assert g["tf_T"] < g["cap_r"].shape[1]
    return 0


if __name__ == "__main__":
    sys.exit(main())
