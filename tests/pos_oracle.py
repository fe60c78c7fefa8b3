"""TEST INFRASTRUCTURE ONLY -- a torch restatement of the POS sequence generator (reference pos_src/SAModel.py,
pos_src/sub_modules.py), eval mode, plus seeded parameters and inputs built on oracle.paramgen.uniform.

Written from reading the reference, not copied: the encoder (sub_modules.py:199-239: Linear -> BN -> ReLU, masked LSTMCell
encoders that ZERO h and c on masked frames, late fusion relu(W [h_rgb ; h_opfl] + b) without gates), init_hidden (SAModel.py:54-60:
the sum of V over all K rows over the mask count), the one-layer attention decoder (sub_modules.py:679-715, unmasked softmax over K)
with the two-input cell (:871-889: order i,f,o,g, the mask holds c and h), the teacher-forced forward with its early break
(SAModel.py:62-90), the pos ClassiferCriterion (SAModel.py:201-218: target rolled left by one) and the greedy rollout that collects
states (SAModel.py:136-184).  tests/golden/pos_*.npz pin it to the reference itself (tools/gen_pos_golden.py).  It runs in the
dtype and on the device of its inputs: float32 on CPU for the fixtures, float64 (on CPU or a GPU through eager torch) as the
high-precision reference of tests/test_gpu_pos_edges.py.
"""
from __future__ import annotations

import collections
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import paramgen as pg  # noqa: E402

PosDims = collections.namedtuple("PosDims", "B K R A E C L F1 F2")

POS_CFG = {
    # deliberately awkward sizes: nothing a multiple of 8 or 32
    "tiny": dict(B=5, K=7, R=24, A=40, E=18, C=5, L=6, F1=20, F2=12),
    # the reference's own sizes (pos_src/myopts.py, run_train.sh --feat_K 20) at batch 8
    "c1": dict(B=8, K=20, R=512, A=1536, E=468, C=20, L=28, F1=1536, F2=1024),
    # mid-size: ragged masks / sentences, and the greedy early exit
    "mid": dict(B=8, K=9, R=64, A=96, E=36, C=20, L=12, F1=48, F2=40),
    # full size (run_train.sh: batch 64, 20 frames, seq_length 28) and the captioner's bench shape
    "full64": dict(B=64, K=20, R=512, A=1536, E=468, C=20, L=28, F1=1536, F2=1024),
    "full128": dict(B=128, K=26, R=512, A=1536, E=468, C=20, L=28, F1=1536, F2=1024),
}
# the greedy early-exit case: a livelier category feedback (embed x15), a wide-variance EOS logit (row 0 of logit.weight x4) and a
# positive EOS bias make some rows finish early and the whole batch exit before seq_length (tools/gen_pos_golden.py checks that the
# reference's top-1/top-2 margin stays >= 1e-3 on every live step)
EOS_CASE = dict(embed_gain=15.0, eos_row_gain=4.0, eos_bias=1.4, input_seed=7)

# golden fixtures tests/golden/pos_<name>.npz: name -> (POS_CFG key, make_inputs kwargs, EOS_CASE weights)
GOLDEN_CASES = {
    "tiny": ("tiny", dict(seed=0), False),
    "c1": ("c1", dict(seed=1), False),
    "ragged": ("mid", dict(seed=2, ragged=True), False),
    "eos": ("mid", dict(seed=EOS_CASE["input_seed"]), True),
    "tfzero": ("tiny", dict(seed=4, ragged=True, max_words=3), False),
}


def make_dims(**kw):
    return PosDims(**kw)


def param_shapes(d):
    """state_dict parameters of the reference POS model, in state_dict order (37 entries)."""
    R, A, E, C = d.R, d.A, d.E, d.C
    s = collections.OrderedDict()
    enc = "two_fc_encoder."
    for m, f in (("rgb", d.F1), ("opfl", d.F2)):
        s[enc + f"visual_emb_{m}.0.weight"] = (R, f)
        s[enc + f"visual_emb_{m}.0.bias"] = (R,)
        s[enc + f"visual_emb_{m}.1.weight"] = (R,)
        s[enc + f"visual_emb_{m}.1.bias"] = (R,)
    for m in ("rgb", "opfl"):
        s[enc + f"lstmcell_{m}.weight_ih"] = (4 * R, R)
        s[enc + f"lstmcell_{m}.weight_hh"] = (4 * R, R)
        s[enc + f"lstmcell_{m}.bias_ih"] = (4 * R,)
        s[enc + f"lstmcell_{m}.bias_hh"] = (4 * R,)
    s[enc + "fusion.late_fusion.0.weight"] = (R, 2 * R)
    s[enc + "fusion.late_fusion.0.bias"] = (R,)
    for n in ("img_embed_h_1", "img_embed_c_1"):
        s[n + ".weight"] = (R, R)
        s[n + ".bias"] = (R,)
    s["lstmcore.lstmcell.i2h.weight"] = (4 * R, E)
    s["lstmcore.lstmcell.i2h.bias"] = (4 * R,)
    s["lstmcore.lstmcell.a2h.weight"] = (4 * R, R)
    s["lstmcore.lstmcell.a2h.bias"] = (4 * R,)
    s["lstmcore.lstmcell.h2h.weight"] = (4 * R, R)
    s["lstmcore.lstmcell.h2h.bias"] = (4 * R,)
    s["lstmcore.v2a.weight"] = (A, R)
    s["lstmcore.v2a.bias"] = (A,)
    s["lstmcore.h2a.weight"] = (A, R)
    s["lstmcore.h2a.bias"] = (A,)
    s["lstmcore.a2w.weight"] = (1, A)
    s["lstmcore.a2w.bias"] = (1,)
    s["embed.weight"] = (C, E)
    s["logit.weight"] = (C, R)
    s["logit.bias"] = (C,)
    return s


def buffer_names():
    out = []
    for m in ("rgb", "opfl"):
        for b in ("running_mean", "running_var", "num_batches_tracked"):
            out.append(f"two_fc_encoder.visual_emb_{m}.1.{b}")
    return out


def state_dict_keys(d):
    """All 43 state_dict keys in the reference's order (the BN buffers follow each BN's affine parameters)."""
    keys = []
    for k in param_shapes(d):
        keys.append(k)
        for m in ("rgb", "opfl"):
            if k == f"two_fc_encoder.visual_emb_{m}.1.bias":
                keys += [f"two_fc_encoder.visual_emb_{m}.1.{b}" for b in ("running_mean", "running_var", "num_batches_tracked")]
    return keys


def make_params(d, seed=1024, logit_gain=8.0, eos=False):
    """U(-1/sqrt(fan_in), 1/sqrt(fan_in)) like nn.Linear, BN affine U(0.5, 1.5) / U(-0.2, 0.2), embed U(-0.1, 0.1); logit.weight
    scaled by `logit_gain` so greedy margins are healthy; `eos`: the EOS_CASE scaling."""
    shapes = param_shapes(d)
    out = collections.OrderedDict()
    for name, shape in shapes.items():
        tag = "pos/" + name
        if name.endswith(".1.weight"):
            out[name] = pg.uniform(tag, shape, seed, 0.5, 1.5)
            continue
        if name.endswith(".1.bias"):
            out[name] = pg.uniform(tag, shape, seed, -0.2, 0.2)
            continue
        if name == "embed.weight":
            out[name] = pg.uniform(tag, shape, seed, -0.1, 0.1)
            continue
        if len(shape) == 2:
            fan_in = shape[1]
        elif name[:-4] + "weight" in shapes:
            fan_in = shapes[name[:-4] + "weight"][1]
        else:                                   # LSTMCell bias_ih / bias_hh
            fan_in = d.R
        b = 1.0 / np.sqrt(float(fan_in))
        if name == "logit.weight":
            b *= logit_gain
        out[name] = pg.uniform(tag, shape, seed, -b, b)
    if eos:
        out["embed.weight"] = out["embed.weight"] * np.float32(EOS_CASE["embed_gain"])
        out["logit.weight"] = out["logit.weight"].copy()
        out["logit.weight"][0] *= np.float32(EOS_CASE["eos_row_gain"])
        out["logit.bias"] = out["logit.bias"].copy()
        out["logit.bias"][0] += np.float32(EOS_CASE["eos_bias"])
    return out


def make_running(d, seed=7):
    """Non-trivial BatchNorm running statistics (eval mode reads them)."""
    out = collections.OrderedDict()
    for m in ("rgb", "opfl"):
        pre = f"two_fc_encoder.visual_emb_{m}.1."
        out[pre + "running_mean"] = pg.uniform("pos/" + pre + "running_mean", (d.R,), seed, -0.3, 0.3)
        out[pre + "running_var"] = pg.uniform("pos/" + pre + "running_var", (d.R,), seed, 0.3, 1.5)
    return out


def make_state_dict(d, P, run):
    sd = collections.OrderedDict()
    for k in state_dict_keys(d):
        if k in P:
            sd[k] = P[k]
        elif k in run:
            sd[k] = run[k]
        else:
            sd[k] = np.array(0, dtype=np.int64)
    return sd


def make_inputs(d, seed=0, ragged=False, max_words=None):
    """features U[0,1); cap_classes (B, L+1) as the reference's collate_fn builds them (pos_src/data_io.py:340-356): categories in
    [1, C) at 0 .. n_b - 1, zero after; class_mask 1 at 0 .. n_b (a few 0 inside the sentence).  `ragged`: varied sentence lengths
    and padded trailing frames on three videos; `max_words` caps every sentence (an all-zero trailing column)."""
    B, K, L = d.B, d.K, d.L
    T = L + 1
    x = {}
    x["feats_rgb"] = pg.uniform("pos/feats_rgb", (B, K, d.F1), seed)
    x["feats_opfl"] = pg.uniform("pos/feats_opfl", (B, K, d.F2), seed)
    feat_mask = np.ones((B, K), dtype=np.float32)
    lens = np.full(B, L, dtype=np.int64)
    if ragged:
        lens = 1 + pg.randint("pos/lens", (B,), seed, 0, L)
        lens[0] = L
        for b in (1, 3, 6):
            if b < B:
                npad = min(4, K - 1) if b != 3 else K - 2
                feat_mask[b, K - npad:] = 0.0
                x["feats_rgb"][b, K - npad:] = 0.0
                x["feats_opfl"][b, K - npad:] = 0.0
    if max_words is not None:
        lens = np.minimum(lens, max_words)
    cats = pg.randint("pos/cats", (B, T), seed, 1, d.C)
    holes = pg.uniform("pos/holes", (B, T), seed) < 0.15
    cap = np.zeros((B, T), dtype=np.int64)
    cmask = np.zeros((B, T), dtype=np.float32)
    for b in range(B):
        n = int(lens[b])
        cap[b, :n] = cats[b, :n]
        cmask[b, :n + 1] = 1.0
        cmask[b, :n][holes[b, :n]] = 0.0
    x["feat_mask"] = feat_mask
    x["cap_classes"] = cap
    x["class_mask"] = cmask
    return x


def prepare_targets(cap_classes, class_mask):
    """starttrain_trainpos.py:132-136 restated: roll the categories right by one (the last column becomes BOS) and set new_mask to
    1 up to and including the last non-zero of class_mask."""
    cap_classes = torch.as_tensor(cap_classes)
    class_mask = torch.as_tensor(class_mask)
    rolled = torch.cat([cap_classes[:, -1:], cap_classes[:, :-1]], dim=1)
    new_mask = torch.zeros_like(class_mask)
    for i in range(class_mask.shape[0]):
        nz = torch.nonzero(class_mask[i] != 0).flatten()
        new_mask[i, :int(nz[-1]) + 1] = 1.0
    return rolled, new_mask


def to_torch(P, dtype=None, device=None):
    """{name: tensor}; `dtype` / `device` (optional) convert the floating-point entries, e.g. float64 on a GPU for a fast
    high-precision reference (the functions below run in the dtype and on the device of their inputs)."""
    out = {}
    for k, v in P.items():
        t = torch.as_tensor(v)
        out[k] = t.to(device=device, dtype=dtype if t.is_floating_point() else None)
    return out


def _lin(x, P, name):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def encoder(P, run, fr, fo, fm, eps=1e-5):
    B, K = fr.shape[:2]
    outs = []
    for m, x in (("rgb", fr), ("opfl", fo)):
        pre = f"two_fc_encoder.visual_emb_{m}."
        z = _lin(x.reshape(B * K, -1), P, pre + "0")
        z = F.batch_norm(z, run[pre + "1.running_mean"], run[pre + "1.running_var"], P[pre + "1.weight"], P[pre + "1.bias"], False,
                         0.0, eps)
        emb = torch.relu(z).reshape(B, K, -1) * fm.unsqueeze(-1)
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
    return torch.relu(_lin(torch.cat(outs, -1), P, "two_fc_encoder.fusion.late_fusion.0"))


def init_hidden(P, V, fm):
    mean = V.sum(1) / fm.sum(1, keepdim=True)
    return _lin(mean, P, "img_embed_h_1"), _lin(mean, P, "img_embed_c_1")


def step(P, V, q, tok, m, h, c):
    """One decoder step: attention on the previous h, the two-input cell, the category head.  m (B, 1)."""
    e = F.linear(torch.tanh(_lin(h, P, "lstmcore.h2a").unsqueeze(1) + q), P["lstmcore.a2w.weight"], P["lstmcore.a2w.bias"])
    alpha = torch.softmax(e, dim=1)
    af = (alpha * V).sum(1)
    s = (_lin(P["embed.weight"][tok], P, "lstmcore.lstmcell.i2h") + _lin(af, P, "lstmcore.lstmcell.a2h") +
         _lin(h, P, "lstmcore.lstmcell.h2h"))
    i, f, o, g = s.chunk(4, 1)
    cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    cn = cn * m + c * (1 - m)
    hn = torch.sigmoid(o) * torch.tanh(cn)
    hn = hn * m + h * (1 - m)
    return hn, cn, F.log_softmax(_lin(hn, P, "logit"), dim=1)


def _prologue(P, run, fr, fo, fm):
    V = encoder(P, run, fr, fo, fm)
    h, c = init_hidden(P, V, fm)
    return V, _lin(V, P, "lstmcore.v2a"), h, c


@torch.no_grad()
def forward_tf(P, run, fr, fo, fm, cap_r, new_mask):
    """(B, T', C) log-probabilities; the loop stops at the first i >= 1 whose category column is all zero."""
    V, q, h, c = _prologue(P, run, fr, fo, fm)
    outs = []
    for i in range(cap_r.shape[1]):
        if i >= 1 and int(cap_r[:, i].sum()) == 0:
            break
        h, c, lp = step(P, V, q, cap_r[:, i], new_mask[:, i:i + 1].to(fr.dtype), h, c)
        outs.append(lp)
    return torch.stack(outs, 1)


def criterion(logp, target, mask, class_mask=None):
    """pos ClassiferCriterion (SAModel.py:201-218): target rolled left by one.  A forward that stopped early (T' < T) is scored on
    the first T' columns of the rolled target and masks."""
    Tp = logp.shape[1]
    target = torch.cat([target[:, 1:], target[:, :1]], 1)[:, :Tp]
    mask = mask[:, :Tp]
    out = -logp.gather(2, target.unsqueeze(2)).squeeze(2) * mask
    if class_mask is None:
        return out.sum() / mask.sum()
    class_mask = class_mask[:, :Tp]
    return (out * class_mask).sum() / (mask * class_mask).sum()


@torch.no_grad()
def sample_greedy(P, run, fr, fo, fm, L):
    """seq (B, n), seqLogprobs (B, n), states (B, n+1, R), masks (B, n+1), and the (n, B, C) log-probabilities each choice was
    made from."""
    V, q, h, c = _prologue(P, run, fr, fo, fm)
    B = fr.shape[0]
    seq, slp, states, masks, lps = [], [], [], [], []
    logp = None
    unf = None
    for t in range(L + 1):
        if t == 0:
            it = torch.zeros(B, dtype=torch.int64, device=fr.device)
            m = torch.ones(B, 1, dtype=fr.dtype, device=fr.device)
        else:
            sl, it = torch.max(logp, 1)
            unf = (it > 0) if t == 1 else unf * (it > 0)
            if int(unf.sum()) == 0:
                break
            seq.append(it * unf.long())
            slp.append(sl)
            lps.append(logp)
            m = unf.to(fr.dtype).unsqueeze(1)
        h, c, logp = step(P, V, q, it, m, h, c)
        states.append(h)
        masks.append(m)
    return (torch.stack(seq, 1), torch.stack(slp, 1), torch.stack(states, 1), torch.cat(masks, 1),
            torch.stack(lps, 0))
