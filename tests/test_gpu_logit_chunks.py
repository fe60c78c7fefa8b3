"""The teacher-forced forward issues the vocabulary product (and, on the fused loss path, the cross-entropy) on the auxiliary stream
in chunks of three decoder steps under the loop, the last chunk ending two steps before the loop does; those two steps' rows follow
on the main stream (xg_model.hip: decoder_fwd_xe, heads_fwd_logits).  B = 32: a chunk is 96 rows, the 4-step last one 128.
T = 21: chunks behind steps 3, 6, 9, 12, 15 and 19, tail 2; T = 9: behind 3 and 7, tail 2; T = 5: one chunk behind step 3, tail 2;
T = 4: one of 2 steps (fewer than a chunk), tail 2; T = 3: no split.
Every case against the fp32 oracle at the suite's fp32 tolerances (tests/util.py, test_gpu_parity.py) and against the same model
without side streams (the bounds of test_single_stream_path_equals_multi_stream_path)."""
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import ws_state as wss
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, assert_grads_close, make_model, model_grads, to_dev

pytestmark = pytest.mark.gpu

STEPS = [21, 9, 5, 4, 3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def dims(T):
    return pg.make_dims(B=32, K=4, R=64, A=96, E=32, V=300, C=6, L=T - 1, F1=48, F2=40, H=128)


@functools.lru_cache(maxsize=None)
def oracle(T):
    """One fp32 oracle forward per T; the gradients of the caption loss alone and of caption + WEIGHT_CLASS * classifier loss."""
    d = dims(T)
    P = xo.to_torch_params(pg.make_params(d), requires_grad=True)
    x = xo.to_torch_inputs(pg.make_inputs(d, seed=0, ragged=True))
    logp, cat, _ = xo.forward_xe(P, x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"],
                                 train=True, running=xo.new_running(d))
    l_xe = xo.lm_criterion(logp, x["seq"], x["seq_mask"])
    l_cls = xo.cls_criterion(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    names, prm = list(P.keys()), list(P.values())

    def grads(loss):
        gs = torch.autograd.grad(loss, prm, retain_graph=True, allow_unused=True)
        return {n: (g.numpy() if g is not None else np.zeros(tuple(q.shape), np.float32)) for n, g, q in zip(names, gs, prm)}
    return dict(logp=logp.detach().numpy(), cat=cat.detach().numpy(), l_xe=l_xe.item(), l_cls=l_cls.item(),
                g_xe=grads(l_xe), g_all=grads(l_xe + WEIGHT_CLASS * l_cls))


def inputs(T):
    x = to_dev(pg.make_inputs(dims(T), seed=0, ragged=True))
    return x, (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])


def fused(T, side_streams=True, classes=False, poison_first=False):
    """xe_loss + backward; returns (model, loss).  poison_first: one iteration to fill the pool, every workspace poisoned, then the
    measured iteration on those workspaces."""
    x, args = inputs(T)
    model = make_model(dims(T))
    if not side_streams:
        model._aux_handle = lambda: None
    extra = (x["cap_classes"], x["class_mask"], WEIGHT_CLASS) if classes else ()
    if poison_first:
        model.xe_loss(*args, *extra).backward()
        torch.cuda.synchronize()
        assert wss.poison_pool(model) >= 1
    model.flat_grads().zero_()
    loss = model.xe_loss(*args, *extra)
    loss.backward()
    torch.cuda.synchronize()
    return model, float(loss.detach())


def same_two_runs(a, b):
    """Two schedules of the same arithmetic (test_single_stream_path_equals_multi_stream_path's bounds)."""
    (ma, la), (mb, lb) = a, b
    assert np.isfinite(lb) and abs(la - lb) <= 5e-6 * max(1.0, abs(la)), (la, lb)
    ga, gb = ma.flat_grads().detach().cpu().numpy(), mb.flat_grads().detach().cpu().numpy()
    assert np.isfinite(gb).all()
    assert np.abs(ga - gb).max() <= 1e-5 * np.abs(ga).max() + 1e-8


@pytest.mark.parametrize("T", STEPS)
def test_fused_loss_path_in_chunks_vs_oracle_and_single_stream(T):
    """cap_classes=None (nobody reads the classifier head): loss within 1e-4, every gradient under grad_misses' three bounds, the
    classifier's gradients exactly zero; and the run without side streams (single split-free schedule) agrees."""
    o = oracle(T)
    run = fused(T)
    model, loss = run
    assert abs(loss - o["l_xe"]) < 1e-4, (loss, o["l_xe"])
    assert_grads_close(model, o["g_xe"], skip=ZERO_GRAD_PARAMS)
    for n, g in model_grads(model).items():
        if n.startswith("classifer."):
            assert not g.any(), n
    same_two_runs(fused(T, side_streams=False), run)


@pytest.mark.parametrize("T", STEPS)
def test_surface_path_in_chunks_vs_oracle_and_single_stream(T):
    """xg_forward_xe (no early loss): log-probs within 3e-4 and category log-probs within 1e-4 of the oracle, as in
    test_xe_forward_backward_vs_oracle; the run without side streams within two runs' round-off (1e-5)."""
    o = oracle(T)
    _, args = inputs(T)
    out = []
    for side in (True, False):
        model = make_model(dims(T))
        if not side:
            model._aux_handle = lambda: None
        with torch.no_grad():
            logp, cat = model(*args)
        torch.cuda.synchronize()
        out.append((logp.cpu().numpy(), cat.cpu().numpy()))
    np.testing.assert_allclose(out[0][0], o["logp"], atol=3e-4, rtol=0)
    np.testing.assert_allclose(out[0][1], o["cat"], atol=1e-4, rtol=0)
    assert np.isfinite(out[0][0]).all()
    np.testing.assert_allclose(out[0][0], out[1][0], atol=1e-5, rtol=0)
    np.testing.assert_allclose(out[0][1], out[1][1], atol=1e-5, rtol=0)


def test_fused_loss_path_with_class_targets_keeps_the_classifier_head():
    """Class targets with weight_class > 0: both losses within 1e-4 and every gradient (the classifier's included) vs the oracle."""
    o = oracle(21)
    model, loss = fused(21, classes=True)
    assert abs(loss - (o["l_xe"] + WEIGHT_CLASS * o["l_cls"])) < 1e-4
    ll = model.last_losses.cpu().numpy()
    assert abs(ll[1] - o["l_xe"]) < 1e-4 and abs(ll[2] - o["l_cls"]) < 1e-4
    assert_grads_close(model, o["g_all"], skip=ZERO_GRAD_PARAMS)
    assert any(g.any() for n, g in model_grads(model).items() if n.startswith("classifer."))


@pytest.mark.parametrize("classes", [False, True])
def test_every_logit_and_lse_row_is_written_on_a_poisoned_workspace(classes):
    """T = 21 on workspaces filled with NaN: an unwritten LOGITS or LSE row would make the loss or the gradients NaN."""
    same_two_runs(fused(21, classes=classes), fused(21, classes=classes, poison_first=True))
