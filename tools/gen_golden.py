#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REFERENCE itself.

Runs only in the build container, where /root/reference exists: imports
caption_src/SAModel.py on CPU (three harness-side shims),
fills it with the procedural weights of oracle/paramgen.py and records small
.npz fixtures (inputs are regenerated from seeds, never stored).  This script
contains no reference code; it only references the path.  Nothing here runs on
the GPU box.

    python tools/gen_golden.py            # writes tests/golden/*.npz
    python tools/gen_golden.py --data-io-only   # only data_io.npz (tests/test_data_cpu.py)
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
from oracle import paramgen as pg  # noqa: E402

REF = "/root/reference/caption_src"
GOLD = os.path.join(ROOT, "tests", "golden")

# dims of the fixtures ------------------------------------------------------------
CFG = {
    # BASELINE.json configs[0]: batch 8, 26 frames, hidden 512, seq_len 20
    "c1": dict(B=8, K=26, R=512, A=1536, E=468, V=20000, C=14, L=20, F1=1536, F2=1024, H=128),
    # deliberately awkward sizes: nothing a multiple of 32, E not a multiple of 4
    "tiny": dict(B=5, K=7, R=24, A=40, E=18, V=61, C=5, L=6, F1=20, F2=12, H=128),
    # BASELINE.json configs[4] shape at small batch (fp32 golden, 1e-2 tol for bf16)
    "c5": dict(B=4, K=40, R=1024, A=1536, E=468, V=20000, C=14, L=6, F1=1536, F2=1024, H=128),
    # mid-size, everything 16-byte aligned (the vector-load kernel paths)
    "mid": dict(B=12, K=9, R=64, A=96, E=36, V=500, C=14, L=7, F1=48, F2=40, H=128),
}
# greedy golden with natural EOS: a livelier token feedback (embed x15) and a wide-variance EOS logit (row 0 of
# logit.weight x4) make the rows emit varied words and finish at different steps; chosen so that the reference's own
# top-1/top-2 margin stays >= 1e-3 on every live step (tests apply the same scaling: tests/util.py:eos_params)
EOS_CASE = dict(embed_gain=15.0, eos_row_gain=4.0, input_seed=2)
WEIGHT_CLASS = 0.5


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


def build_ref(ref, d, P, p_drop=0.0):
    opt = argparse.Namespace(seed=1024, vocab_size=d.V, category_size=d.C,
                             input_encoding_size=d.E, rnn_size=d.R, num_layers=1,
                             drop_prob_lm=p_drop, seq_length=d.L, feat_size=d.F1,
                             feat_size2=d.F2, att_size=d.A, fusion_activity="ReLU")
    model = ref.SAModel(opt)
    sd = {k: torch.from_numpy(v.copy()) for k, v in P.items()}
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys, missing
    assert all("running" in k or "num_batches" in k for k in missing.missing_keys), missing
    return model


def tt(x):
    return {k: torch.from_numpy(v) for k, v in x.items()}


def sample_idx(name, shape, n=16):
    tot = int(np.prod(shape))
    return (pg.hash_u32(7, zlib_crc(name), 3, n).astype(np.int64) % tot)


def zlib_crc(s):
    import zlib
    return zlib.crc32(s.encode()) & 0xFFFFFFFF


def grads_summary(model, full=False):
    out = {}
    for name, prm in model.named_parameters():
        g = prm.grad
        if g is None:
            g = torch.zeros_like(prm)
        g = g.detach().numpy()
        out["gnorm/" + name] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        out["gsamp/" + name] = g.reshape(-1)[sample_idx(name, g.shape)].copy()
        if full:
            out["gfull/" + name] = g.copy()
    return out


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def gen_xe(ref, tag, ragged, full):
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0, ragged=ragged))
    model = build_ref(ref, d, P)
    model.train()
    steps = []
    hook = model.lstmcore.register_forward_hook(
        lambda m, i, o: steps.append([o[1][0][0][0].detach().numpy().copy(), o[1][0][1][0].detach().numpy().copy(),
                                      o[1][1][0][0].detach().numpy().copy(), o[1][1][1][0].detach().numpy().copy()]))
    enc_out = []
    h2 = model.two_spatial_encoder.register_forward_hook(lambda m, i, o: enc_out.append(o.detach().numpy().copy()))
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    hook.remove(); h2.remove()
    crit, ccrit = ref.LanguageModelCriterion(), ref.ClassiferCriterion()
    l_xe = crit(logp, x["seq"], x["seq_mask"])
    l_cls = ccrit(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    loss = l_xe + WEIGHT_CLASS * l_cls
    model.zero_grad()
    loss.backward()
    g = {}
    g["loss_xe"] = np.float64(l_xe.item()); g["loss_cls"] = np.float64(l_cls.item())
    g["loss"] = np.float64(loss.item())
    lp = logp.detach().numpy()
    ns = lp.shape[2] if full else 32
    g["logp_slice"] = lp[:, :, :ns].copy()
    tgt = torch.cat([x["seq"][:, 1:], x["seq"][:, :1]], 1)
    g["logp_tgt"] = logp.detach().gather(2, tgt.unsqueeze(2)).squeeze(2).numpy()
    g["cat_logp"] = cat.detach().numpy()
    st = np.array(steps)                       # (T,4,B,R)
    nr = st.shape[-1] if full else 16
    g["state_slice"] = st[:, :, :, :nr].copy()
    g["V_slice"] = enc_out[0][:, :, :nr].copy()
    # BN running stats after ONE train-mode forward (momentum 0.1, unbiased var)
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        g[f"bn_{mod}_running_mean"] = bn.running_mean.numpy().copy()
        g[f"bn_{mod}_running_var"] = bn.running_var.numpy().copy()
    g.update(grads_summary(model, full))
    name = f"xe_{tag}{'_ragged' if ragged else ''}.npz"
    np.savez_compressed(os.path.join(GOLD, name), **g)
    print("wrote", name, "loss", g["loss"])


# logit gain of the greedy goldens (oracle/paramgen.py:make_params): chosen per config so that the reference's own top-1 / top-2
# margin is >= 1e-3 on every decoded step; recorded in the fixture, the tests read it from there
GREEDY_GAIN = {"tiny": 8.0, "c1": 24.0}


def gen_greedy(ref, tag, ragged=False):
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d, logit_gain=GREEDY_GAIN[tag])
    x = tt(pg.make_inputs(d, seed=0, ragged=ragged))
    model = build_ref(ref, d, P)
    model.eval()          # eval.py:73 / eval_utils.py:25: running stats at their init (0,1)
    logps = []
    hook = model.logit.register_forward_hook(lambda m, i, o: logps.append(torch.log_softmax(o, 1).detach().numpy().copy()))
    with quiet(), torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    hook.remove()
    lp = np.array(logps)                                      # (n+1, B, V)
    top2 = -np.sort(-lp, axis=2)[:, :, :2]
    g = dict(seq=seq.numpy(), seqLogprobs=slp.numpy(), margin=(top2[:, :, 0] - top2[:, :, 1]), logit_gain=np.float32(GREEDY_GAIN[tag]))
    g["min_margin"] = np.float32(g["margin"][: seq.shape[1]].min())
    name = f"greedy_{tag}{'_ragged' if ragged else ''}.npz"
    np.savez_compressed(os.path.join(GOLD, name), **g)
    print("wrote", name, "n", seq.shape[1], "min margin", g["min_margin"])
    assert g["min_margin"] >= 1e-3


def eos_params(d):
    P = pg.make_params(d)
    P["embed.weight"] = P["embed.weight"] * np.float32(EOS_CASE["embed_gain"])
    P["logit.weight"] = P["logit.weight"].copy()
    P["logit.weight"][0] *= np.float32(EOS_CASE["eos_row_gain"])
    return P


def gen_greedy_eos(ref):
    """Greedy decode (SAModel.py:163-219, eval mode) where rows finish naturally at different steps: pins the
    `unfinished` bookkeeping (:200-215), the zeroing of finished rows (:208) and the state hold under xt_mask."""
    d = pg.make_dims(**CFG["c1"])
    P = eos_params(d)
    x = tt(pg.make_inputs(d, seed=EOS_CASE["input_seed"]))
    model = build_ref(ref, d, P)
    model.eval()
    logps = []
    hook = model.logit.register_forward_hook(lambda m, i, o: logps.append(torch.log_softmax(o, 1).detach().numpy().copy()))
    with quiet(), torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    hook.remove()
    s = seq.numpy()
    lp = np.array(logps)[: s.shape[1]]
    top2 = -np.sort(-lp, axis=2)[:, :, :2]
    margin = top2[:, :, 0] - top2[:, :, 1]                     # (n, B): margin of the choice made at step t+1
    alive = np.ones_like(margin, bool)
    for b in range(d.B):
        z = np.flatnonzero(s[b] == 0)
        if z.size:
            alive[z[0] + 1:, b] = False
    g = dict(seq=s, seqLogprobs=slp.numpy(), margin=margin, alive=alive)
    np.savez_compressed(os.path.join(GOLD, "greedy_c1_eos.npz"), **g)
    lens = [int(np.flatnonzero(s[b] == 0)[0]) if (s[b] == 0).any() else -1 for b in range(d.B)]
    print("wrote greedy_c1_eos.npz n", s.shape[1], "distinct tokens", len(np.unique(s)), "EOS at", lens,
          "min live margin", margin[alive].min())
    assert margin[alive].min() >= 1e-3 and len(np.unique(s)) > 30 and sum(1 for v in lens if 2 <= v <= 15) >= 4


def gen_traj(ref, tag, iters=3):
    """f-1 / a11: the reference model under the reference's update rule -- optim.Adam(model.parameters(), lr) with torch
    defaults (starttrain.py:76), loss = L_xe + weight_class * L_cls (:125-129), backward (:134), elementwise clamp of
    every gradient to +-grad_clip = 0.1 (myutils.py:79-85; py2-only file, its three-line loop is restated here), step
    (:137) -- three iterations on one batch.  Records the losses and the parameters afterwards."""
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0, ragged=True))
    model = build_ref(ref, d, P)
    model.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=4e-4, weight_decay=0.0)
    crit, ccrit = ref.LanguageModelCriterion(), ref.ClassiferCriterion()
    losses = []
    for _ in range(iters):
        optimizer.zero_grad()
        logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
        loss = crit(logp, x["seq"], x["seq_mask"]) + WEIGHT_CLASS * ccrit(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
        loss.backward()
        for group in optimizer.param_groups:                       # myutils.clip_gradient
            for prm in group["params"]:
                if prm.grad is not None:
                    prm.grad.data.clamp_(-0.1, 0.1)
        optimizer.step()
        losses.append(loss.item())
    g = dict(losses=np.array(losses, np.float64), lr=np.float64(4e-4), grad_clip=np.float64(0.1))
    for name, prm in model.named_parameters():
        v = prm.detach().numpy()
        g["pnorm/" + name] = np.float64(np.sqrt((v.astype(np.float64) ** 2).sum()))
        g["pidx/" + name] = sample_idx(name, v.shape, 256)
        g["psamp/" + name] = v.reshape(-1)[g["pidx/" + name]].copy()
        g["dsamp/" + name] = (v.reshape(-1)[g["pidx/" + name]] - P[name].reshape(-1)[g["pidx/" + name]]).copy()
        if tag == "tiny":
            g["pfull/" + name] = v.copy()
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        g[f"bn_{mod}_running_mean"] = bn.running_mean.numpy().copy()
        g[f"bn_{mod}_running_var"] = bn.running_var.numpy().copy()
    np.savez_compressed(os.path.join(GOLD, f"traj_{tag}.npz"), **g)
    print("wrote", f"traj_{tag}.npz", "losses", losses)


def gen_step(ref):
    """G5: one LSTMCore_two_layer_gate step from a random state, B=4, c1 sizes."""
    cfg = dict(CFG["c1"]); cfg["B"] = 4
    d = pg.make_dims(**cfg)
    P = pg.make_params(d)
    model = build_ref(ref, d, P)
    model.train()
    B, K, R, E = d.B, d.K, d.R, d.E
    xt = torch.from_numpy(pg.uniform("step.xt", (B, E), 5, -0.1, 0.1))
    V = torch.from_numpy(pg.uniform("step.V", (B, K, R), 5, 0.0, 1.0))
    pos = torch.from_numpy(pg.uniform("step.pos", (B, R), 5, -1.0, 1.0))
    st = [torch.from_numpy(pg.uniform(f"step.s{i}", (1, B, R), 5, -0.5, 0.5)) for i in range(4)]
    mk = torch.tensor([[1.0], [1.0], [0.0], [1.0]])
    alphas = []
    hk = model.lstmcore.a2w.register_forward_hook(lambda m, i, o: alphas.append(torch.softmax(o, 1).squeeze(-1).detach().numpy().copy()))
    out, state = model.lstmcore(xt, mk, V, pos, [(st[0], st[1]), (st[2], st[3])])
    hk.remove()
    g = dict(out=out.detach().numpy(), h1=state[0][0][0].detach().numpy(), c1=state[0][1][0].detach().numpy(),
             h2=state[1][0][0].detach().numpy(), c2=state[1][1][0].detach().numpy(), alpha=alphas[0])
    np.savez_compressed(os.path.join(GOLD, "step_c1.npz"), **g)
    print("wrote step_c1.npz")


def gen_scst(ref, tag):
    """G6: SCST replay.  The reference samples with torch.multinomial on the CPU
    generator (SAModel.py:190-194); the sampled tokens are recorded and replayed."""
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0))
    model = build_ref(ref, d, P)
    model.train()                                            # starttrain.py:68 (never toggled)
    torch.manual_seed(1234)
    with quiet():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 0})
    reward_b = pg.uniform("reward", (d.B,), 3, -1.0, 1.0)
    reward = torch.from_numpy(np.repeat(reward_b[:, None], seq.shape[1], 1))   # myutils.py:76
    loss = ref.RewardCriterion()(slp, seq, reward)
    model.zero_grad()
    loss.backward()
    g = dict(seq=seq.numpy(), seqLogprobs=slp.detach().numpy(), reward=reward.numpy(), loss=np.float64(loss.item()))
    g.update(grads_summary(model, full=(tag == "tiny")))
    np.savez_compressed(os.path.join(GOLD, f"scst_{tag}.npz"), **g)
    print("wrote", f"scst_{tag}.npz", "n", seq.shape[1], "loss", g["loss"])


def gen_eval_bn(ref, tag):
    """G8: eval-mode forward with non-trivial running statistics."""
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0, ragged=True))
    model = build_ref(ref, d, P)
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        bn.running_mean.copy_(torch.from_numpy(pg.uniform(f"rm.{mod}", (d.R,), 9, -0.3, 0.3)))
        bn.running_var.copy_(torch.from_numpy(pg.uniform(f"rv.{mod}", (d.R,), 9, 0.5, 2.0)))
    model.eval()
    with torch.no_grad():
        logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
        loss = ref.LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    g = dict(loss=np.float64(loss.item()), logp_slice=logp.numpy()[:, :, :32].copy(), cat_logp=cat.numpy())
    np.savez_compressed(os.path.join(GOLD, f"evalbn_{tag}.npz"), **g)
    print("wrote", f"evalbn_{tag}.npz", "loss", g["loss"])


def gen_ss(ref, tag):
    """f-3: scheduled sampling (SAModel.py:89-99) with ss_prob = 0.5; the tokens fed to embed at every step are
    recorded (the draws come from torch's global RNG) and replayed by the oracle."""
    d = pg.make_dims(**CFG[tag])
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0, ragged=True))
    model = build_ref(ref, d, P)
    model.train()
    model.ss_prob = 0.5
    its = []
    hk = model.embed.register_forward_hook(lambda m, i, o: its.append(i[0].detach().numpy().copy()))
    torch.manual_seed(4321)
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    hk.remove()
    loss = ref.LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    model.zero_grad(); loss.backward()
    its = np.array(its)                                        # (T,B)
    g = dict(it=its, loss=np.float64(loss.item()), n_replaced=np.int64((its != x["seq"].numpy().T).sum()))
    g.update(grads_summary(model, full=False))
    np.savez_compressed(os.path.join(GOLD, f"ss_{tag}.npz"), **g)
    print("wrote", f"ss_{tag}.npz", "loss", g["loss"], "replaced tokens", g["n_replaced"])


def gen_beam(ref, tag, beam_size=3):
    """f-2: beam search (CaptionModel.py:22-128) tokens / logps, eval mode."""
    cfg = dict(CFG[tag]); cfg["B"] = min(cfg["B"], 3)
    d = pg.make_dims(**cfg)
    P = pg.make_params(d)
    x = tt(pg.make_inputs(d, seed=0))
    model = build_ref(ref, d, P)
    model.eval()
    with quiet(), torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                {"beam_size": beam_size})
    g = dict(seq=seq.numpy(), seqLogprobs=slp.numpy(), beam_size=np.int64(beam_size))
    np.savez_compressed(os.path.join(GOLD, f"beam_{tag}.npz"), **g)
    print("wrote", f"beam_{tag}.npz")


def gen_decode():
    """myutils.decode_sequence (caption_src/myutils.py:88-102) is host-only string work in a py2 file that py3 cannot
    import (print statement at module level): the function's own lines are exec'd from where they lie, on an (N, D)
    token matrix behind a shim that hands out Python ints like torch 0.3 did.  Fixture: tokens + expected strings."""
    import json
    src = open(os.path.join(REF, "myutils.py")).read().splitlines()
    i0 = next(i for i, l in enumerate(src) if l.startswith("def decode_sequence"))
    i1 = next(i for i in range(i0 + 1, len(src)) if src[i] and not src[i][0].isspace())
    ns = {}
    exec("\n".join(src[i0:i1]), ns)

    class IntMatrix:
        def __init__(self, a): self.a = a
        def size(self): return self.a.shape
        def __getitem__(self, ij): return int(self.a[ij])

    rng = np.random.RandomState(5)
    seq = rng.randint(1, 40, size=(9, 7)).astype(np.int64)
    seq[0, 3:] = 0; seq[1, 0] = 0; seq[2, 6] = 0; seq[3, 1] = 0; seq[3, 4] = 7; seq[5, 2:5] = 0; seq[7, :] = 0
    vocab = {i: "w%d" % i for i in range(1, 40)}
    vocab[3] = "a"; vocab[7] = "<unk>"; vocab[11] = "it's"
    want = ns["decode_sequence"](vocab, IntMatrix(seq))
    with open(os.path.join(GOLD, "decode_seq.json"), "w") as f:
        json.dump({"seq": seq.tolist(), "vocab": {str(k): v for k, v in vocab.items()}, "sents": want}, f)
    print("wrote decode_seq.json", want[:4])


def gen_data_io():
    """caption_src/data_io.py on the inputs of tests/test_data_cpu.py (regenerated there from the same seeds): get_sub_frames,
    collate_fn, custom_dset_train / custom_dset_test item by item and filt_word_category tag by tag.  Fixture: data_io.npz."""
    import argparse
    import pickle
    import tempfile
    from tests import test_data_cpu as td
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, REF)
    argv, sys.argv = sys.argv, ["x"]                       # (myopts parses the command line at import)
    import data_io as ref
    sys.argv = argv
    g = {}
    rng = np.random.default_rng(2)
    for n in td.SUB_FRAME_LENGTHS:
        g["sub_frames_%d" % n] = ref.get_sub_frames(rng.random((n, 8)).astype(np.float32), 26)
    items = td._items(rng)
    batch = [("vid%d_0" % i, it["cap"], it["cap_class"], it["class_mask"], it["feat1"], it["feat2"], it["feat_mask"],
              it["pos_feat"], np.zeros((1, 3))) for i, it in enumerate(items)]
    for i, t in enumerate(ref.collate_fn(batch)[1:9]):
        g["collate_%d" % i] = t.numpy()
    split, caps, worddict, category, f1, f2, pos = td._corpus(np.random.default_rng(4))
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for name, obj in (("split", split), ("caps", caps), ("wd", worddict), ("cate", category)):
            paths[name] = os.path.join(tmp, name + ".pkl")
            with open(paths[name], "wb") as f:
                pickle.dump(obj, f)
        for kind, Ref in (("train", ref.custom_dset_train), ("test", ref.custom_dset_test)):
            r = Ref(paths["split"], paths["caps"], paths["cate"], f1, f2, pos, paths["wd"], K=10, opt=argparse.Namespace(seq_length=6))
            g["%s_ids" % kind] = np.array(r.data_list)
            for i in range(len(r)):
                for key, v in zip(td.ITEM_KEYS, r[i]):
                    g["%s_%d_%s" % (kind, i, key)] = np.asarray(v.numpy() if torch.is_tensor(v) else v)
        cate = os.path.join(tmp, "cate.pkl")
        with open(cate, "wb") as f:
            pickle.dump({t: ["w%d" % i] for i, t in enumerate(td.POS_TAGS)}, f)
        words = ["w%d" % i for i in range(len(td.POS_TAGS))] + ["untagged"]
        theirs = ref.filt_word_category(cate, {w: i + 2 for i, w in enumerate(words)})[0]
    g["pos_tag_category"] = np.array([theirs["w%d" % i] for i in range(len(td.POS_TAGS))], np.int64)
    g["pos_untagged_category"] = np.int64(theirs.get("untagged", 1))
    np.savez_compressed(os.path.join(GOLD, "data_io.npz"), **g)
    print("wrote data_io.npz", len(g), "arrays")


def main():
    if not os.path.isdir(REF):
        print("reference not present; nothing to do")
        return 0
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(8)
    if "--decode-only" in sys.argv:
        gen_decode()
        return 0
    if "--data-io-only" in sys.argv:
        gen_data_io()
        return 0
    round2_only = "--round2-only" in sys.argv          # (import_reference() resets sys.argv for the reference's argparse)
    greedy_only = "--greedy-only" in sys.argv
    ref = import_reference()
    if greedy_only:          # round 5: the config-1 greedy goldens at a logit gain that gives >= 1e-3 margins
        gen_greedy(ref, "tiny")
        gen_greedy(ref, "c1")
        gen_greedy(ref, "c1", ragged=True)
        return 0
    if round2_only:          # the fixtures added in round 2 (the older ones regenerate bit-identically)
        gen_greedy_eos(ref)
        gen_traj(ref, "tiny")
        gen_traj(ref, "mid")
        gen_decode()
        return 0
    gen_xe(ref, "tiny", ragged=False, full=True)
    gen_xe(ref, "tiny", ragged=True, full=True)
    gen_xe(ref, "c1", ragged=False, full=False)
    gen_xe(ref, "c1", ragged=True, full=False)
    gen_xe(ref, "c5", ragged=False, full=False)
    gen_greedy(ref, "tiny")
    gen_greedy(ref, "c1")
    gen_greedy(ref, "c1", ragged=True)
    gen_step(ref)
    gen_scst(ref, "tiny")
    gen_scst(ref, "c1")
    gen_eval_bn(ref, "tiny")
    gen_eval_bn(ref, "c1")
    gen_beam(ref, "tiny")
    gen_beam(ref, "c1")
    gen_ss(ref, "tiny")
    gen_greedy_eos(ref)
    gen_traj(ref, "tiny")
    gen_traj(ref, "mid")
    gen_decode()
    gen_data_io()
    return 0


if __name__ == "__main__":
    sys.exit(main())
