"""The POS sequence generator on the MI355X: PosModel's HIP forward and greedy rollout against the reference's own outputs
(tests/golden/pos_*.npz), against tests/pos_oracle.py at full size, eval-mode dropout, determinism, and the extraction feeding the
captioner end to end."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import pos_oracle as po
from tests.util import CFG, ROOT, assert_greedy_tokens_match, make_model

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def make_opt(d, drop_prob_lm=0.0):
    return argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1,
                              drop_prob_lm=drop_prob_lm, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)


def pos_model(d, P, run, drop_prob_lm=0.0):
    from controllable_xgating_amd.pos import PosModel
    m = PosModel(make_opt(d, drop_prob_lm))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    return m.cuda().eval()


def cuda_inputs(x):
    return [torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask")]


def run_model(m, x):
    from controllable_xgating_amd.pos import ClassiferCriterion, prepare_pos_targets
    args = cuda_inputs(x)
    cap_r, new_mask = prepare_pos_targets(torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"]))
    cap_r, new_mask, cm = cap_r.cuda(), new_mask.cuda(), torch.from_numpy(x["class_mask"]).cuda()
    with torch.no_grad():
        out = m(*args, None, None, cap_r, new_mask)
        loss = float(ClassiferCriterion()(out, cap_r, new_mask, cm))
        seq, slp, states, masks = m.sample(*args, {"sample_max": 1})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in
            dict(tf_logp=out, loss=loss, seq=seq, seqLogprobs=slp, states=states, masks=masks).items()}


def check_against(h, o, margin, lp_tol=3e-4, loss_tol=1e-4, st_tol=1e-4):
    """h: this implementation, o: the reference (golden) or the oracle; margin (n, B): top-1 / top-2 margin of each choice."""
    assert h["tf_logp"].shape == o["tf_logp"].shape
    np.testing.assert_allclose(h["tf_logp"], o["tf_logp"], atol=lp_tol)
    if o.get("loss") is not None:
        assert abs(h["loss"] - float(o["loss"])) < loss_tol
    g_h, g_o = h["seq"], o["seq"]
    lps = [np.stack([np.array([0.0, m]) for m in margin[t]])[None] for t in range(margin.shape[0])]   # (1, B, 2) per step
    assert_greedy_tokens_match(g_h, g_o, [torch.from_numpy(a[0]) for a in lps])
    # states, masks and log-probs up to the first step where a near-tie went the other way (everywhere when none did)
    n = min(g_h.shape[1], g_o.shape[1])
    diff = np.flatnonzero((g_h[:, :n] != g_o[:, :n]).any(0))
    k = int(diff[0]) if diff.size else n
    if g_h.shape == g_o.shape and not diff.size:
        np.testing.assert_allclose(h["masks"], o["masks"], atol=st_tol)
        if "pos_feat" in o:
            np.testing.assert_allclose(h["states"][:, n], o["pos_feat"], atol=st_tol)
    np.testing.assert_allclose(h["seqLogprobs"][:, :k], o["seqLogprobs"][:, :k], atol=lp_tol)
    cols = o["states"].shape[2]
    np.testing.assert_allclose(h["states"][:, :k + 1, :cols], o["states"][:, :k + 1], atol=st_tol)
    np.testing.assert_allclose(h["masks"][:, :k + 1], o["masks"][:, :k + 1], atol=st_tol)


def oracle_outputs(d, P, run, x):
    Pt, rt = po.to_torch(P), po.to_torch(run)
    fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    out = po.forward_tf(Pt, rt, fr, fo, fm, cap_r, new_mask)
    loss = po.criterion(out, cap_r, new_mask, torch.from_numpy(x["class_mask"]))
    seq, slp, states, masks, lps = po.sample_greedy(Pt, rt, fr, fo, fm, d.L)
    top2 = torch.topk(lps, 2, dim=2).values
    o = dict(tf_logp=out.numpy(), loss=float(loss), seq=seq.numpy(), seqLogprobs=slp.numpy(), states=states.numpy(),
             masks=masks.numpy())
    return o, (top2[:, :, 0] - top2[:, :, 1]).numpy()


@pytest.mark.parametrize("name", list(po.GOLDEN_CASES))
def test_matches_reference_goldens(name):
    cfg, kw, eos = po.GOLDEN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **kw)
    g = dict(np.load(os.path.join(GOLD, "pos_%s.npz" % name)))
    h = run_model(pos_model(d, P, run), x)
    check_against(h, g, g["margin"])
    assert h["tf_logp"].shape[1] == int(g["tf_T"])


@pytest.mark.parametrize("cfg", ["full64", "full128"])
def test_full_size_against_oracle(cfg):
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=11, ragged=True)
    h = run_model(pos_model(d, P, run), x)
    o, margin = oracle_outputs(d, P, run, x)
    check_against(h, o, margin)


def test_eval_dropout_is_the_identity():
    d = po.make_dims(**po.POS_CFG["mid"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=2, ragged=True)
    a = run_model(pos_model(d, P, run, 0.0), x)
    b = run_model(pos_model(d, P, run, 0.5), x)
    for k in ("tf_logp", "seq", "seqLogprobs", "states", "masks"):
        assert np.array_equal(a[k], b[k]), k
    assert a["loss"] == b["loss"]


def test_two_identical_calls_are_bit_identical():
    d = po.make_dims(**po.POS_CFG["c1"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=5, ragged=True)
    m = pos_model(d, P, run)
    a, b = run_model(m, x), run_model(m, x)
    for k in ("tf_logp", "seq", "seqLogprobs", "states", "masks"):
        assert np.array_equal(a[k], b[k]), k
    assert a["loss"] == b["loss"]


def test_inference_only_model_is_never_flattened():
    """An eval-mode PosModel reads every parameter through its own pointer: forward, sample and sample_forced allocate no flat
    or gradient buffer and rebind no parameter."""
    d = po.make_dims(**po.POS_CFG["tiny"])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, seed=3, ragged=True)
    m = pos_model(d, P, run)
    ptrs = [p.data_ptr() for p in m.parameters()]
    h = run_model(m, x)                                          # forward and sample
    tag_logp, _, _, pos_feats = m.sample_forced(*cuda_inputs(x), [[[2, 4, 1], [3]]] * d.B)
    torch.cuda.synchronize()
    assert np.isfinite(h["tf_logp"]).all() and torch.isfinite(tag_logp).all() and torch.isfinite(pos_feats).all()
    assert [p.data_ptr() for p in m.parameters()] == ptrs
    assert m._flat is None and m._gflat is None and all(p.grad is None for p in m.parameters())


def test_extraction_feeds_the_captioner_end_to_end():
    """extract_pos_features over two batches into a dict -> data.make_video_item picks each video's last state row -> the
    captioner's greedy SAModel.sample on those vectors, against the oracle chain (pos_oracle -> oracle.xgate_oracle)."""
    from controllable_xgating_amd.data import make_video_item
    from controllable_xgating_amd.pos import extract_pos_features
    dp = po.make_dims(**po.POS_CFG["mid"])           # K 9, R 64, F1 48, F2 40: the captioner's "mid" shape
    dc = pg.make_dims(**CFG["mid"])
    assert (dp.K, dp.R, dp.F1, dp.F2) == (dc.K, dc.R, dc.F1, dc.F2)
    P, run = po.make_params(dp), po.make_running(dp)
    m = pos_model(dp, P, run)
    xs = [po.make_inputs(dp, seed=20, ragged=True), po.make_inputs(dp, seed=21)]
    ids = [["v%d" % i for i in range(dp.B)], ["v%d" % i for i in range(dp.B - 2, 2 * dp.B - 2)]]   # two ids repeat: first wins
    batches = [(*cuda_inputs(x), torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"]), v) for x, v in zip(xs, ids)]
    writer = {}
    loss = extract_pos_features(m, batches, writer)
    assert len(writer) == 2 * dp.B - 2
    # the oracle chain
    Pt, rt = po.to_torch(P), po.to_torch(run)
    want, losses = {}, []
    for x, v in zip(xs, ids):
        fr, fo, fm = (torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
        cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
        out = po.forward_tf(Pt, rt, fr, fo, fm, cap_r, new_mask)
        losses.append(float(po.criterion(out, cap_r, new_mask, torch.from_numpy(x["class_mask"]))))
        seq, _, states, masks, _ = po.sample_greedy(Pt, rt, fr, fo, fm, dp.L)
        for i, vid in enumerate(v):
            want.setdefault(vid, (x, i, states[i].numpy(), masks[i].numpy(), seq[i].numpy()))
    assert abs(loss - np.mean(losses)) < 1e-4
    items, pos_o = [], []
    for vid in sorted(writer, key=lambda s: int(s[1:]))[:dc.B]:
        x, i, st, mk, sq = want[vid]
        grp = writer[vid]
        assert grp["states"].shape == st.shape and grp["masks"].shape == (1, mk.shape[0]) and grp["tokens"].shape == (1, sq.shape[0])
        np.testing.assert_allclose(grp["states"], st, atol=1e-4)
        items.append(make_video_item(x["feats_rgb"][i], x["feats_opfl"][i], grp["states"], dc.K))
        pos_o.append(st[-1])
    f1 = torch.stack([it[0] for it in items]).cuda()
    f2 = torch.stack([it[1] for it in items]).cuda()
    fm = torch.cat([it[2] for it in items]).cuda()
    pos = torch.stack([it[3] for it in items]).cuda()
    np.testing.assert_allclose(pos.cpu().numpy(), np.stack(pos_o), atol=1e-4)
    Pc = pg.make_params(dc)
    cap = make_model(dc, Pc, train=False)
    with torch.no_grad():
        seq_h, _ = cap.sample(f1, f2, fm, pos, {"sample_max": 1})
        seq_o, _, lps = xo.sample(xo.to_torch_params(Pc), f1.cpu(), f2.cpu(), fm.cpu(), torch.from_numpy(np.stack(pos_o)), dc.L,
                                  mode="greedy", train=False, running=xo.new_running(dc), return_logp=True)
    assert_greedy_tokens_match(seq_h.cpu().numpy(), seq_o.numpy(), lps)
