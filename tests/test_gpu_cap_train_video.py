"""Teacher-forced training on Q captions per video on the MI355X: SAModel.xe_loss_per_video (include/xgate_train_video.h) against
the composed oracle of tests/cap_train_video_oracle.py -- loss, both criteria, every parameter gradient and the BatchNorm running
statistics, no row and no parameter excused --, against xe_loss on the repeated batch, under dropout, in eval mode, on a workspace
full of NaNs, and through Trainer.train_batch.

Bounds (tests/test_gpu_parity.py): loss and each criterion 1e-4, gradients by assert_grads_close's defaults (rtol 2e-3, atol 2e-6,
cosine >= 1 - 1e-5), running statistics atol 1e-5; under dropout loss 2e-4 and gradients rtol 3e-3; parameters after two iterations
atol 2e-5.  The cases and what each reaches: tests/cap_train_video_oracle.py, checked without a GPU in
tests/test_cap_train_video_cpu.py."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import xgate_oracle as xo
from tests import cap_train_video_oracle as tvo
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, assert_grads_close, make_model, model_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The device inputs of a case in the order xe_loss_per_video takes them (made once, shared, never changed)."""
    d, Q, _, xv, xr = tvo.case_inputs(name)
    T = d.L + 1
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    cls = tvo.CASES[name][3]
    return (t(xv["feats_rgb"]), t(xv["feats_opfl"]), t(xv["feat_mask"]), t(xr["pos_feats"]).reshape(d.B, Q, d.R),
            t(xr["seq"]).reshape(d.B, Q, T), t(xr["seq_mask"]).reshape(d.B, Q, T),
            t(xr["cap_classes"]).reshape(d.B, Q, T) if cls else None, t(xr["class_mask"]).reshape(d.B, Q, T) if cls else None,
            WEIGHT_CLASS if cls else 0.0)


def _repeated(name):
    a = _dev(name)
    Q = a[3].shape[1]
    flat = lambda t: None if t is None else t.reshape(-1, *t.shape[2:])      # noqa: E731
    return tuple(t.repeat_interleave(Q, 0) for t in a[:3]) + tuple(flat(t) for t in a[3:8]) + (a[8],)


def _model(name, p=0.0, seed=None, train=True):
    d, _, P = tvo.case_inputs(name)[:3]
    m = make_model(d, P, p_drop=p, train=train)
    if seed is not None:
        m.dropout_seed = seed
    return m


def _step(model, name, zero=True):
    """loss.backward() of one per-video call; returns (loss, last_losses) as floats."""
    if zero:
        model.zero_grad(set_to_none=True)
    loss = model.xe_loss_per_video(*_dev(name))
    loss.backward()
    torch.cuda.synchronize()
    ll = model.last_losses.cpu().numpy()
    return float(loss.item()), ll


def _check_running(model, running):
    for mod in ("rgb", "opfl"):
        bn = getattr(model.two_spatial_encoder, f"visual_emb_{mod}")[1]
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), running[pre + "running_mean"].numpy(), atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), running[pre + "running_var"].numpy(), atol=1e-5)
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("name", ["tiny", "odd", "one_q1", "one_q5", "mid", "c1", "c5", "mid_q224"])
def test_loss_gradients_and_running_statistics_vs_composed_oracle(name):
    ref = tvo.case_reference(name)
    model = _model(name)
    loss, ll = _step(model, name)
    print("%s: loss %.6f (oracle %.6f), lm %.6f (%.6f), cls %.6f (%.6f)" % (name, loss, ref["loss"], ll[1], ref["lm"], ll[2], ref["cls"]))
    assert abs(loss - ref["loss"]) < 1e-4 and abs(ll[0] - ref["loss"]) < 1e-4
    assert abs(ll[1] - ref["lm"]) < 1e-4 and abs(ll[2] - ref["cls"]) < 1e-4
    report = {}
    try:
        assert_grads_close(model, ref["grads"], report=report)
    finally:
        worst = max(report.items(), key=lambda kv: kv[1][2]) if report else None
        print("%s: worst gradient %s" % (name, worst))
    _check_running(model, ref["running"])


@pytest.mark.parametrize("name", ["mid", "c1", "mid_q1"])
def test_equals_xe_loss_on_the_repeated_batch(name):
    """p = 0: the per-video call against xe_loss on repeat_interleave'd inputs (mid_q1: Q = 1, the same batch) -- the same loss and
    gradients within the bounds above."""
    a, b = _model(name), _model(name)
    loss_a, ll_a = _step(a, name)
    loss = b.xe_loss(*_repeated(name))
    loss.backward()
    torch.cuda.synchronize()
    ll_b = b.last_losses.cpu().numpy()
    print("%s: per-video %.6f, repeated %.6f" % (name, loss_a, loss.item()))
    assert abs(loss_a - loss.item()) < 1e-4 and np.abs(ll_a - ll_b).max() < 1e-4
    assert_grads_close(a, model_grads(b))
    ra, rb = (m.two_spatial_encoder.visual_emb_rgb[1] for m in (a, b))
    np.testing.assert_allclose(ra.running_mean.cpu().numpy(), rb.running_mean.cpu().numpy(), atol=1e-5)
    if name == "mid_q1":
        np.testing.assert_allclose(ra.running_var.cpu().numpy(), rb.running_var.cpu().numpy(), atol=1e-5)


def test_dropout_masks_match_the_composed_oracle():
    """p = 0.5, fixed seed: the encoder's sites draw by element index in the B-video tensors, the decoder's and the heads' by row in
    the M-row tensors -- the composed oracle under ONE seed (bounds of test_dropout_masks_match_oracle_hash)."""
    name, seed = "mid_q3", 123457
    ref = tvo.case_reference(name, True, 0.5, seed)
    model = _model(name, p=0.5, seed=seed)
    loss, ll = _step(model, name)
    print("dropout: loss %.6f (oracle %.6f)" % (loss, ref["loss"]))
    assert abs(loss - ref["loss"]) < 2e-4 and abs(ll[1] - ref["lm"]) < 2e-4 and abs(ll[2] - ref["cls"]) < 2e-4
    assert_grads_close(model, ref["grads"], rtol=3e-3)
    other = _model(name, p=0.5, seed=seed + 1)
    with torch.no_grad():
        l2 = float(other.xe_loss_per_video(*_dev(name)).item())
    assert abs(l2 - loss) > 1e-3, (l2, loss)


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_eval_mode_forward_vs_oracle(name):
    ref = tvo.case_reference(name, False)
    model = _model(name, train=False)
    with torch.no_grad():
        loss = float(model.xe_loss_per_video(*_dev(name)).item())
    ll = model.last_losses.cpu().numpy()
    assert abs(loss - ref["loss"]) < 1e-4 and abs(ll[1] - ref["lm"]) < 1e-4 and abs(ll[2] - ref["cls"]) < 1e-4
    bn = model.two_spatial_encoder.visual_emb_rgb[1]
    assert int(bn.num_batches_tracked) == 0 and float(bn.running_mean.abs().max()) == 0.0


def _video_grads(model):
    """dvproj (B,K,A) and dV (B,K,R) of the last backward, formed again from its workspace (xgtv_video_grads)."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_train_video as ntv
    from controllable_xgating_amd.model import _stream, _ws_ptr
    d, Q, ws = model._last_video_ws
    wp, wn = _ws_ptr(ws)
    dvproj = torch.empty(d.B, d.K, d.A, device="cuda")
    dV = torch.empty(d.B, d.K, d.R, device="cuda")
    nv.check(ntv.lib().xgtv_video_grads(_stream(), C.byref(d), Q, C.byref(model._params_struct()), wp, wn, nv.ptr(dvproj), nv.ptr(dV)),
             "xgtv_video_grads")
    torch.cuda.synchronize()
    return dvproj, dV


@pytest.mark.parametrize("name", ["mid", "odd"])
def test_nan_filled_workspace_gives_the_results_of_a_zeroed_one(name):
    model = _model(name)
    _step(model, name)                                       # the first call allocates the workspace; the next ones reuse it
    ws = model._last_video_ws[2]
    out = []
    for fill in (0, 255):                                    # 0xFF bytes: every float a NaN
        ws.fill_(fill)
        loss, ll = _step(model, name)
        assert model._last_video_ws[2] is ws
        out.append((loss, ll, model_grads(model), _video_grads(model)))
    (l0, ll0, g0, v0), (l1, ll1, g1, v1) = out
    assert np.isfinite(l1) and abs(l0 - l1) <= 1e-6 and np.abs(ll0 - ll1).max() <= 1e-6
    for n, g in g1.items():
        assert np.isfinite(g).all(), n
    assert_grads_close(model, g0)
    for a, b in zip(v0, v1):
        assert bool(torch.isfinite(b).all())
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=2e-3, atol=2e-6 + 2e-4 * float(a.abs().max()))


@pytest.mark.parametrize("name", ["mid", "c1", "odd", "mid_q224"])
def test_video_sums_have_one_writer_and_a_fixed_order(name):
    """dvproj and dV: formed twice from the same saved tensors, bit for bit the same (one writer per element, the Q T terms in a
    fixed order, no float atomics); and they are the sums over q that the definition gives, from the per-row tensors."""
    model = _model(name)
    _step(model, name)
    a, b = _video_grads(model), _video_grads(model)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0


def test_two_identical_calls_give_bit_identical_video_sums():
    """Two identical calls (same parameters, inputs and workspace contents): dvproj and dV bit for bit.  The case is the generic
    step (R = 20, no packed weights), whose per-step products feed the sums in one order; what the existing reverse-time pass
    accumulates by float atomics in its packed form (docs/CAPTION_TRAIN_PER_VIDEO.md) is not part of this check."""
    name = "odd"
    model = _model(name)
    out = []
    for _ in range(2):
        _step(model, name)
        out.append(_video_grads(model))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_identical_captions_of_one_video_give_the_q_fold_sums():
    """mid: the Q captions of video 2 are identical rows, so the per-video sums of that video are Q times what ONE of its rows
    sends.  That one row's share comes from a Q = 1 call on the same B videos (the same BatchNorm batch, hence the same V) with
    every video's first caption: a video's sums depend on its own rows only."""
    name = "mid"
    d, Q, P, xv, xr = tvo.case_inputs(name)
    b = tvo.IDENTICAL_VIDEO[name]
    model = _model(name)
    _step(model, name)
    dvproj, dV = _video_grads(model)
    # every row's share of the loss is 1 / (sum of ALL masks): the Q = 1 call is scaled to the same denominator through dloss
    # (the language-model and the classifier criterion share the mask here: class_mask is all ones, so one scale serves both)
    args = _dev(name)
    assert bool((args[7] == 1).all())
    one = args[:3] + tuple(None if t is None else t[:, :1].contiguous() for t in args[3:8]) + (args[8],)
    m1 = _model(name)
    loss = m1.xe_loss_per_video(*one)
    scale = float(args[5][:, 0].sum() / args[5].sum())
    (loss * scale).backward()
    torch.cuda.synchronize()
    dvproj1, dV1 = _video_grads(m1)
    for whole, single in ((dvproj[b], dvproj1[b]), (dV[b], dV1[b])):
        ref = (Q * single).cpu().numpy()
        np.testing.assert_allclose(whole.cpu().numpy(), ref, rtol=2e-3, atol=2e-6 + 2e-4 * np.abs(ref).max())


def _trainer(model, overlap=True):
    from controllable_xgating_amd.driver import Trainer
    opt = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, weight_class=WEIGHT_CLASS, overlap_update=overlap,
                             learning_rate_decay_start=-1, scheduled_sampling_start=-1, self_critical_after=-1)
    tr = Trainer(model, opt)
    tr.start_epoch(0)
    return tr


def _batch(args):
    return dict(feat1=args[0], feat2=args[1], feat_mask=args[2], pos_feat=args[3], cap=args[4], cap_mask=args[5], cap_classes=args[6],
                class_mask=args[7])


def _params_close(a, b):
    pb = dict(b.named_parameters())
    for name, prm in a.named_parameters():
        if name in ZERO_GRAD_PARAMS:      # round-off of cancelling terms, which Adam turns into +-lr steps (test_gpu_parity.py)
            continue
        np.testing.assert_allclose(prm.detach().cpu().numpy(), pb[name].detach().cpu().numpy(), atol=2e-5, err_msg=name)


def test_trainer_two_iterations_move_the_parameters_as_the_repeated_batch_does():
    name = "mid"
    a, b, c = _model(name), _model(name), _model(name)
    ta, tb, tc = _trainer(a), _trainer(b), _trainer(c, overlap=False)
    la = [float(ta.train_batch(_batch(_dev(name)))["loss"].item()) for _ in range(2)]
    lb = [float(tb.train_batch(_batch(_repeated(name)))["loss"].item()) for _ in range(2)]
    lc = [float(tc.train_batch(_batch(_dev(name)))["loss"].item()) for _ in range(2)]
    torch.cuda.synchronize()
    print("trainer: per-video %s, repeated %s, per-video without overlap %s" % (la, lb, lc))
    np.testing.assert_allclose(la, lb, atol=2e-4)
    np.testing.assert_allclose(la, lc, atol=2e-4)
    assert la[1] < la[0]
    _params_close(a, b)
    _params_close(a, c)                   # overlap_update on and off
