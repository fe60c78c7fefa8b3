"""The POS sequence generator's side of joint training on the MI355X (include/xgate_pos_joint.h; docs/JOINT_TRAINING.md):
xgpj_final_state -- the state the captioner consumes, out of the train-mode forward's workspace -- and xgpj_backward -- the backward
with that state's gradient as one more input --, against the float64 oracle of tests/joint_oracle.py, and PosModel.forward(...,
return_pos_feats=True) on top of them.

Bounds, all existing ones: states within 1e-4 and log-probabilities within 3e-4 (tests/test_gpu_pos_train.py), every parameter gradient
by pos_train_oracle.golden_grad_misses at its defaults."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import joint_oracle as jo
from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import grad_misses

pytestmark = pytest.mark.gpu

SEED = 1357
# What the existing backward accumulates by float atomics (xg_pointwise.hip: the embedding scatter-add; xg_attn.hip: a2w.weight in the
# attention's post pass): two runs of xgpt_backward itself differ there in their last bits (measured: up to 4.7e-10)
ATOMIC_GRADS = ("embed.weight", "lstmcore.a2w.weight")
# name -> (POS_CFG key, make_inputs kwargs): pos_train_oracle.TRAIN_CASES' inputs, the dropout probability is the test's
CASES = {"tiny": ("tiny", dict(seed=0)), "ragged": ("mid", dict(seed=2, ragged=True)), "tfzero": ("tiny", dict(seed=4, ragged=True, max_words=3))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg, kw = CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    return d, po.make_params(d), po.make_running(d), po.make_inputs(d, **kw)


@functools.lru_cache(maxsize=None)
def _w(name):
    """The fixed random weights of the objective sum(w * pos_feats)."""
    d = _case(name)[0]
    return np.random.default_rng(77).standard_normal((d.B, d.R)).astype(np.float32)


def _model(name, p=0.0, train=True):
    from controllable_xgating_amd.pos import PosModel
    d, P, run, _ = _case(name)
    opt = argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1, drop_prob_lm=p,
                             seq_length=d.L, feat_size=d.F1, feat_size2=d.F2)
    m = PosModel(opt)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in po.make_state_dict(d, P, run).items()}, strict=True)
    m = m.cuda().train(train)
    m.dropout_seed = SEED
    return m


def _batch(name):
    from controllable_xgating_amd.pos import prepare_pos_targets
    x = _case(name)[3]
    fr, fo, fm = (torch.from_numpy(x[k]).cuda() for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = prepare_pos_targets(torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"]))
    return fr, fo, fm, cap_r.cuda(), new_mask.cuda(), torch.from_numpy(x["class_mask"]).cuda()


# ---- 4. the final state
@pytest.mark.parametrize("name", ["ragged", "tfzero"])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_final_state_in_train_mode_equals_the_oracles_last_state(name, p):
    d, P, run, x = _case(name)
    m = _model(name, p)
    fr, fo, fm, cap_r, new_mask, _ = _batch(name)
    logp, pos = m(fr, fo, fm, None, None, cap_r, new_mask, return_pos_feats=True)
    assert pos.requires_grad and logp.requires_grad and tuple(pos.shape) == (d.B, d.R)
    ref = jo.pos_reference(d, P, run, x, p, SEED)
    assert logp.shape[1] == ref["logp"].shape[1] and (logp.shape[1] < d.L + 1) == (name == "tfzero")
    np.testing.assert_allclose(logp.detach().cpu().numpy(), ref["logp"], atol=3e-4)
    np.testing.assert_allclose(pos.detach().cpu().numpy(), ref["state"], atol=1e-4)
    if name == "ragged":
        # rows that ended early are held: their last state is an earlier step's, and under dropout it keeps that step's mask
        ends = x["class_mask"].shape[1] - 1 - np.argmax(x["class_mask"][:, ::-1] != 0, axis=1)
        assert (ends < logp.shape[1] - 1).any()
    # the default returns what it returned before
    out = _model(name, p)(fr, fo, fm, None, None, cap_r, new_mask)
    assert torch.is_tensor(out)
    np.testing.assert_allclose(out.detach().cpu().numpy(), logp.detach().cpu().numpy(), atol=3e-4)


def _forward_direct(m, name, train):
    """xgpt_forward_train with XgptRun.train as given (PosModel's eval mode runs another entry point): (dims, run, Tp, logp)."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos_train as npt
    from controllable_xgating_amd._plumbing import _stream
    d = _case(name)[0]
    fr, fo, fm, cap_r, new_mask, _ = _batch(name)
    dims = m._dims(d.B, d.K, d.L + 1)
    m._ensure_flat()
    ws = m._train_workspace(dims, fr.device)
    run = m._run()
    run.train = 1 if train else 0
    logp = torch.empty(d.B, d.L + 1, d.C, device="cuda")
    t_out = torch.empty(1, dtype=torch.int32, device="cuda")
    P, bn = m._params(), m._bn()
    nv.check(npt.lib().xgpt_forward_train(_stream(), C.byref(dims), C.byref(P), C.byref(bn), C.byref(run), fr.data_ptr(), fo.data_ptr(),
                                          fm.data_ptr(), cap_r.data_ptr(), new_mask.float().contiguous().data_ptr(), logp.data_ptr(),
                                          t_out.data_ptr(), ws.data_ptr(), ws.numel()), "xgpt_forward_train")
    return dims, run, int(t_out.item()), logp, ws, (fr, fo, fm)


def _final_state(dims, Tp, ws, B, R):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos_joint as npj
    from controllable_xgating_amd._plumbing import _stream
    pos = torch.full((B, R), float("nan"), device="cuda")
    nv.check(npj.lib().xgpj_final_state(_stream(), C.byref(dims), Tp, ws.data_ptr(), ws.numel(), pos.data_ptr()), "xgpj_final_state")
    torch.cuda.synchronize()
    return pos


@pytest.mark.parametrize("name", ["ragged", "tfzero"])
def test_final_state_without_train_mode_equals_sample_forced_on_the_same_tags(name):
    """XgptRun.train = 0 (running statistics, no dropout): the state behind step T' - 1 is the vector sample_forced returns for the same
    tags -- the generator rolled along them to the end, finished rows held -- and the float64 oracle's."""
    d, P, run, x = _case(name)
    m = _model(name, 0.5, train=False)
    dims, _, Tp, _, ws, _ = _forward_direct(m, name, train=False)
    pos = _final_state(dims, Tp, ws, d.B, d.R)
    templates = torch.from_numpy(x["cap_classes"][:, :d.L]).cuda()
    with torch.no_grad():
        forced = m.sample_forced(*_batch(name)[:3], templates)[3]
    assert tuple(forced.shape) == (d.B, d.R)
    np.testing.assert_allclose(pos.cpu().numpy(), forced.cpu().numpy(), atol=1e-4)
    ref = jo.pos_reference(d, P, run, x, 0.5, SEED, with_logp=False, train=False)
    np.testing.assert_allclose(pos.cpu().numpy(), ref["state"], atol=1e-4)


# ---- 5. the backward
def _backward_direct(m, entry, dims, run, Tp, ws, feats, dlogp, dpos):
    """One backward into a fresh gradient buffer: {name: tensor}.  entry "xgpt": xgpt_backward (dpos must be None)."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_joint as npj
    from controllable_xgating_amd import _native_pos_train as npt
    from controllable_xgating_amd._plumbing import _stream
    g = torch.zeros_like(m.flat_parameters())
    gs = m._struct_of(g)
    fr, fo, fm = feats
    P = m._params()
    dl = None if dlogp is None else dlogp.data_ptr()
    if entry == "xgpt":
        assert dpos is None
        nv.check(npt.lib().xgpt_backward(_stream(), C.byref(dims), C.byref(P), C.byref(gs), C.byref(run), fr.data_ptr(), fo.data_ptr(),
                                         fm.data_ptr(), Tp, dl, ws.data_ptr(), ws.numel()), "xgpt_backward")
    else:
        nv.check(npj.lib().xgpj_backward(_stream(), C.byref(dims), C.byref(P), C.byref(gs), C.byref(run), fr.data_ptr(), fo.data_ptr(),
                                         fm.data_ptr(), Tp, dl, ws.data_ptr(), ws.numel(), None if dpos is None else dpos.data_ptr()),
                 "xgpj_backward")
    torch.cuda.synchronize()
    return {n: v.clone() for n, v in zip(npos.PARAM_NAMES, m._grad_views(g))}


def _as_fixture(grads):
    return {"g/" + n: np.asarray(v, np.float64) for n, v in grads.items()}


@pytest.mark.parametrize("name,p", [("tiny", 0.0), ("ragged", 0.5), ("tfzero", 0.0)])
def test_backward_in_three_settings_against_float64(name, p):
    from controllable_xgating_amd.pos import ClassiferCriterion
    d, P, run, x = _case(name)
    m = _model(name, p)
    dims, xrun, Tp, logp, ws, feats = _forward_direct(m, name, train=True)
    _, _, _, cap_r, new_mask, cm = _batch(name)
    # the criterion's gradient for the log-probabilities of the T' steps, from the project's own criterion
    leaf = logp[:, :Tp].contiguous().requires_grad_(True)
    ClassiferCriterion()(leaf, cap_r, new_mask, cm).backward()
    dlogp = leaf.grad.contiguous()
    w = torch.from_numpy(_w(name)).cuda()
    cpu = lambda g: {n: v.cpu().numpy() for n, v in g.items()}      # noqa: E731
    # (a) dlogp only: xgpt_backward bit for bit -- but for the two gradients it sums by float atomics, which are held to grad_misses'
    # defaults against it -- and the oracle's gradient of the criterion
    old = _backward_direct(m, "xgpt", dims, xrun, Tp, ws, feats, dlogp, None)
    new = _backward_direct(m, "xgpj", dims, xrun, Tp, ws, feats, dlogp, None)
    diff = [n for n in old if n not in ATOMIC_GRADS and not torch.equal(old[n], new[n])]
    assert not diff, diff
    bad = grad_misses({n: new[n].cpu().numpy() for n in ATOMIC_GRADS}, {n: old[n].cpu().numpy() for n in ATOMIC_GRADS})
    assert not bad, bad
    ref_a = jo.pos_reference(d, P, run, x, p, SEED)
    miss = pto.golden_grad_misses(cpu(new), _as_fixture(ref_a["grads"]))
    assert not miss, ("dlogp only", miss)
    # (b) dpos only: dlogp NULL, the objective sum(w * pos_feats)
    only = _backward_direct(m, "xgpj", dims, xrun, Tp, ws, feats, None, w)
    ref_b = jo.pos_reference(d, P, run, x, p, SEED, w_pos=_w(name), with_logp=False)
    miss = pto.golden_grad_misses(cpu(only), _as_fixture(ref_b["grads"]))
    assert not miss, ("dpos only", miss)
    assert float(only["logit.weight"].abs().max()) == 0.0 and float(only["logit.bias"].abs().max()) == 0.0
    assert float(only["lstmcore.lstmcell.h2h.weight"].abs().max()) > 0
    # (c) both
    both = _backward_direct(m, "xgpj", dims, xrun, Tp, ws, feats, dlogp, w)
    ref_c = jo.pos_reference(d, P, run, x, p, SEED, w_pos=_w(name))
    miss = pto.golden_grad_misses(cpu(both), _as_fixture(ref_c["grads"]))
    assert not miss, ("both", miss)


@pytest.mark.parametrize("with_logp", [True, False])
def test_posmodel_autograd_carries_both_gradients(with_logp):
    """PosModel.forward(..., return_pos_feats=True) through loss.backward(): the criterion plus sum(w * pos_feats), and the latter
    alone -- the backward then receives None for dlogp and the head's gradients are exactly zero."""
    from controllable_xgating_amd.pos import ClassiferCriterion
    name, p = "ragged", 0.5
    d, P, run, x = _case(name)
    m = _model(name, p)
    fr, fo, fm, cap_r, new_mask, cm = _batch(name)
    logp, pos = m(fr, fo, fm, None, None, cap_r, new_mask, return_pos_feats=True)
    loss = (torch.from_numpy(_w(name)).cuda() * pos).sum()
    if with_logp:
        loss = loss + ClassiferCriterion()(logp, cap_r, new_mask, cm)
    loss.backward()
    torch.cuda.synchronize()
    got = {n: (q.grad if q.grad is not None else torch.zeros_like(q)).detach().cpu().numpy() for n, q in m.named_parameters()}
    ref = jo.pos_reference(d, P, run, x, p, SEED, w_pos=_w(name), with_logp=with_logp)
    assert abs(loss.item() - ref["loss"]) < 1e-4 * max(1.0, abs(ref["loss"]))
    miss = pto.golden_grad_misses(got, _as_fixture(ref["grads"]))
    assert not miss, miss
    if not with_logp:
        assert np.abs(got["logit.weight"]).max() == 0.0 and np.abs(got["logit.bias"]).max() == 0.0


def test_return_pos_feats_is_refused_in_eval_mode():
    m = _model("tiny", train=False)
    fr, fo, fm, cap_r, new_mask, _ = _batch("tiny")
    with pytest.raises(NotImplementedError, match="sample_forced"):
        m(fr, fo, fm, None, None, cap_r, new_mask, return_pos_feats=True)
    assert torch.is_tensor(m(fr, fo, fm, None, None, cap_r, new_mask))
