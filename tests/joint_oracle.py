"""TEST INFRASTRUCTURE ONLY -- the float64 oracle of joint training (docs/JOINT_TRAINING.md), composed from the existing oracles
without editing them: oracle/xgate_oracle.py (through the compositions of tests/cap_ss_oracle.py) for the captioner and
tests/pos_train_oracle.py (encoder, step, mask, params, running) for the POS sequence generator.

  * pos_forward: the generator's train-mode forward as its own loop over `step`, stopping where forward_train stops, that also
    returns the state behind the last step that ran -- the vector the captioner consumes;
  * caption_reference: a captioner loss of any of the four fused forms with pos_feats as a LEAF, so that autograd yields
    d loss / d pos_feats next to the parameter gradients;
  * joint_loss: L_cap(pos_feats(P_pos)) + lambda * L_pos, one graph over both models' parameters;
  * the shared shapes and inputs of tests/test_joint_cpu.py and the GPU tests (made once, never changed).
"""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import cap_ss_oracle as sso
from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import CFG, WEIGHT_CLASS, oracle_f64_with_flips

# the tiny shape of both models: the generator's POS_CFG["tiny"] and the captioner at the same B, K, R (and A, E, C, L, F1, F2) with
# a small vocabulary.  Both libraries accept R = 24 (a multiple of 8: the captioner's LDS-staged step, the four-wide dpos kernel).
POS_TINY = po.POS_CFG["tiny"]
CAP_TINY = dict(CFG["tiny"])
assert all(CAP_TINY[k] == POS_TINY[k] for k in ("B", "K", "R", "A", "E", "C", "L", "F1", "F2"))
# the second shape of the dpos tests: R % 4 != 0 (the scalar kernel); nothing aligned
CAP_ODD = dict(CFG["odd"], R=18)


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ the generator
def _lin(x, P, name):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def pos_forward(P, run, fr, fo, fm, cap_r, new_mask, p=0.0, seed=0, train=True):
    """(logp (B,T',C), last state (B,R)): pos_train_oracle.forward_train's loop with the state kept.  The state is the one behind
    step T' - 1, after the step's dropout mask (held rows included): what the loop carries.  train=False: eval-mode BatchNorm over
    `run`, no dropout."""
    pd = p if train else 0.0
    V = pto.encoder(P, run, fr, fo, fm, pd, seed, None, train)
    with torch.no_grad():
        mean = (V.sum(1) / fm.sum(1, keepdim=True)).detach()
    h, c = _lin(mean, P, "img_embed_h_1"), _lin(mean, P, "img_embed_c_1")
    q = _lin(V, P, "lstmcore.v2a")
    B, R = h.shape
    outs = []
    for i in range(cap_r.shape[1]):
        if i >= 1 and int(cap_r[:, i].sum()) == 0:
            break
        keep = pto.mask(seed, pto.SITE_CELL, i, (B, R), pd, fr.dtype, fr.device)
        h, c, lp = pto.step(P, V, q, cap_r[:, i], new_mask[:, i:i + 1].to(fr.dtype), h, c, keep)
        outs.append(lp)
    return torch.stack(outs, 1), h


def pos_reference(d, P, run, x, p=0.0, seed=0, w_pos=None, with_logp=True, train=True):
    """One float64 forward of the generator and the gradients of  [with_logp] ClassiferCriterion(logp) + [w_pos] sum(w_pos * state)
    with respect to every parameter: dict(logp, state, loss, grads).  Parameters without a path get zeros."""
    dt = torch.float64
    Pt, rt = pto.params(P, dt), pto.running(run, dt)
    fr, fo, fm = (torch.from_numpy(x[k]).to(dt) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    logp, h = pos_forward(Pt, rt, fr, fo, fm, cap_r, new_mask.to(dt), p, seed, train)
    loss = torch.zeros((), dtype=dt)
    if with_logp:
        loss = loss + pto.criterion(logp, cap_r, new_mask.to(dt), torch.from_numpy(x["class_mask"]).to(dt))
    if w_pos is not None:
        loss = loss + (torch.from_numpy(np.asarray(w_pos)).to(dt) * h).sum()
    grads = None
    if loss.requires_grad:
        loss.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in Pt.items()}
    return dict(logp=logp.detach().numpy(), state=h.detach().numpy(), loss=loss.item(), grads=grads)


# ------------------------------------------------------------------------------------------------ the captioner
def caption_fn(d, Q, cls, p, seed, holder, forced=None, scale=1.0):
    """run_oracle's fn for a fused caption loss with pos_feats as a leaf: the composition of tests/cap_ss_oracle.py (rows = B max(Q, 1);
    at Q = 0 it is the plain loss without forward_xe's early stop -- all T steps run, as on the device, and a step at which every row is
    padding adds nothing to the loss).  `forced` (T, M): the fed tokens under scheduled sampling.  `scale`: a non-unit dloss.  The leaf
    of the call that ran with gradients is left in holder["pos"]."""
    forced_t = None if forced is None else torch.from_numpy(np.ascontiguousarray(forced)).long()

    def fn(P, xi, tr):
        xi = dict(xi)
        pos = xi["pos_feats"].detach().clone().requires_grad_(torch.is_grad_enabled())
        xi["pos_feats"] = pos
        running = xo.new_running(d)
        logp, cat = sso.forward(P, xi, d, max(Q, 1), True, p, seed, running, forced_it=forced_t, relu_trace=tr)
        loss, lm, lc = sso.losses(logp, cat, xi, cls)
        if torch.is_grad_enabled():
            holder["pos"] = pos
        return loss * scale, (lm.item(), lc.item(), running)

    return fn


def caption_reference(P, x, d, Q, cls, p=0.0, seed=0, forced=None, scale=1.0):
    """(loss, parameter gradients {name: float64 ndarray}, ReLU-flip exemptions for them, dpos (M,R) float64 ndarray) of the float64
    oracle.  x: the videos' feats_rgb / feats_opfl / feat_mask and the rows' pos_feats, seq, seq_mask, cap_classes, class_mask."""
    holder = {}
    loss, _, g64, ex = oracle_f64_with_flips(P, x, caption_fn(d, Q, cls, p, seed, holder, forced, scale))
    return loss, g64, ex, holder["pos"].grad.double().numpy()


# ------------------------------------------------------------------------------------------------ both
@functools.lru_cache(maxsize=None)
def joint_case(seed=5):
    """(d_cap, d_pos, P_cap, P_pos, run_pos, x) at the tiny shape: x holds the features, feat_mask, cap_classes and class_mask of the
    generator's inputs (ragged) and seq / seq_mask of the captioner's (ragged).  numpy, never changed."""
    dc, dp = pg.make_dims(**CAP_TINY), po.make_dims(**POS_TINY)
    xp = po.make_inputs(dp, seed=seed, ragged=True)
    xc = pg.make_inputs(dc, seed=0, ragged=True)
    x = dict(xp, seq=xc["seq"], seq_mask=xc["seq_mask"])
    return dc, dp, pg.make_params(dc), po.make_params(dp), po.make_running(dp), x


def joint_loss(Pc, Pp, run_p, x, dc, lam, p=0.0, seed_c=0, seed_p=0, detach=False):
    """L_cap(pos_feats(P_pos)) + lam * L_pos in the dtype of the tensors handed in (Pc, Pp: {name: tensor}; run_p is updated in
    place).  The generator's criterion takes the captions' mask, as PosTrainer does when the batch carries cap_mask.  Returns (loss,
    L_cap, L_pos)."""
    dt = next(iter(Pp.values())).dtype
    with default_dtype(dt):
        fr, fo, fm = (torch.from_numpy(x[k]).to(dt) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
        cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
        seq, seq_mask = torch.from_numpy(x["seq"]), torch.from_numpy(x["seq_mask"]).to(dt)
        cm = torch.from_numpy(x["class_mask"]).to(dt)
        logp_pos, pos = pos_forward(Pp, run_p, fr, fo, fm, cap_r, new_mask.to(dt), p, seed_p)
        l_pos = pto.criterion(logp_pos, cap_r, seq_mask, cm)
        xi = dict(feats_rgb=fr, feats_opfl=fo, feat_mask=fm, pos_feats=pos.detach() if detach else pos, seq=seq, seq_mask=seq_mask,
                  cap_classes=torch.from_numpy(x["cap_classes"]), class_mask=cm)
        logp, cat = sso.forward(Pc, xi, dc, 1, True, p, seed_c, xo.new_running(dc))
        l_cap, _, _ = sso.losses(logp, cat, xi, True)
        return l_cap + lam * l_pos, l_cap, l_pos


def joint_grads(Pc_np, Pp_np, run_np, x, dc, lam, detach=False):
    """The float64 composed gradient: (loss, L_cap, L_pos, {name: ndarray} for the captioner, the same for the generator)."""
    dt = torch.float64
    Pc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dt).requires_grad_(True) for k, v in Pc_np.items()}
    Pp = pto.params(Pp_np, dt)
    loss, lc, lp = joint_loss(Pc, Pp, pto.running(run_np, dt), x, dc, lam, detach=detach)
    loss.backward()
    g = lambda P: {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}      # noqa: E731
    return loss.item(), lc.item(), lp.item(), g(Pc), g(Pp)


def joint_trajectory(lam, steps, lr, clip):
    """`steps` iterations of joint training in float64 from joint_case(): every parameter of both models after each iteration, as
    pos_train_oracle.traj_misses reads them -- ({"p<it>/<name>": ndarray} for the captioner, the same for the generator, losses)."""
    dc, dp, Pc, Pp, run, x = joint_case()
    Pc = {k: np.asarray(v, np.float64) for k, v in Pc.items()}
    Pp = {k: np.asarray(v, np.float64) for k, v in Pp.items()}
    sc, sp, gc, gp, losses = {}, {}, {}, {}, []
    for it in range(steps):
        loss, _, _, dPc, dPp = joint_grads(Pc, Pp, run, x, dc, lam)
        losses.append(loss)
        Pc = {k: np.asarray(v, np.float64) for k, v in pto.clip_adam(Pc, dPc, sc, it + 1, lr, clip).items()}
        Pp = {k: np.asarray(v, np.float64) for k, v in pto.clip_adam(Pp, dPp, sp, it + 1, lr, clip).items()}
        gc.update({"p%d/%s" % (it, k): v for k, v in Pc.items()})
        gp.update({"p%d/%s" % (it, k): v for k, v in Pp.items()})
    return gc, gp, losses
