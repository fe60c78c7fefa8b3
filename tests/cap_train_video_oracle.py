"""The oracle of teacher-forced training on Q captions per video (include/xgate_train_video.h; test infrastructure): the pieces of
oracle.xgate_oracle composed the way SAModel.xe_loss_per_video is defined --

    encoder_fwd, init_hidden and v2a on the B videos; V, v2a(V) and the initial state repeated to the M = B Q rows; the core_step /
    heads loop of forward_xe on the M rows; loss = lm_criterion + weight_class * cls_criterion over the M rows

-- with ONE dropout seed: the encoder's sites then draw by element index in the B-video tensors and the decoder's and the heads' by
row in the M-row tensors.  Also the cases of tests/test_gpu_cap_train_video.py, their inputs (made once, never changed) and what each
case reaches."""
import functools

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG, WEIGHT_CLASS

GROUP = 4            # csrc/xg_kernels.h: XGK_ATTN_BWD_GROUP = XGCC_TEMPLATE_GROUP, rows of one video per workgroup of the fast forms

# name -> (CFG entry, B, Q, with the classifier term)
CASES = {
    "tiny": ("tiny", 5, 3, True),        # ragged seq_mask per caption, ragged feat_mask; one caption all padding behind BOS
    "odd": ("odd", 3, 2, True),          # R = 20: generic step; A = 37: the rows form of the per-step attention backward
    "one_q1": ("one", 1, 1, False),      # K = 1, T = 2
    "one_q5": ("one", 1, 5, False),      # ... and a partial group behind a full one
    "mid": ("mid", 4, 5, True),          # aligned fast forms, Q no multiple of the group size; video 2's captions identical
    "mid_q3": ("mid", 4, 3, True),       # the dropout case
    "mid_q1": ("mid", 4, 1, True),       # Q = 1 against xe_loss
    "c1": ("c1", 2, 4, False),           # real layer sizes, K = 26, V = 20000
    "c5": ("c5", 2, 2, False),           # K = 40 > 32, R = 1024: the group kernel's second block of q and second batch of V pieces
    "mid_q224": ("mid", 1, 224, False),  # 56 groups of one video; the post-loop pass walks 112 chunks, a frame per workgroup
}
IDENTICAL_VIDEO = {"mid": 2}
PADDED_ROW = {"tiny": (1, 2)}            # (video, caption): only BOS is fed and counted


def dims(name):
    cfg, B, Q, _ = CASES[name]
    return pg.make_dims(**dict(CFG[cfg], B=B)), Q


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(d, Q, P, xv, xr): d with d.B = videos, the parameters, the videos' inputs (feats_rgb, feats_opfl, feat_mask) and the rows'
    (pos_feats (M,R), seq, seq_mask, cap_classes, class_mask (M,T)), row b Q + q.  numpy, never changed."""
    d, Q = dims(name)
    M = d.B * Q
    P = pg.make_params(d)
    v = pg.make_inputs(d, seed=0, ragged=True)
    r = pg.make_inputs(d._replace(B=M), seed=1, ragged=True)
    xv = {k: v[k] for k in ("feats_rgb", "feats_opfl", "feat_mask")}
    xr = {k: r[k].copy() for k in ("pos_feats", "seq", "seq_mask", "cap_classes", "class_mask")}
    if name in PADDED_ROW:
        b, q = PADDED_ROW[name]
        xr["seq"][b * Q + q, 1:] = 0
        xr["seq_mask"][b * Q + q, 1:] = 0.0
    if name in IDENTICAL_VIDEO:
        b = IDENTICAL_VIDEO[name]
        for k in xr:
            xr[k][b * Q:(b + 1) * Q] = xr[k][b * Q]
    assert (xr["seq"][:, 1:].sum(0) > 0).all()         # no step at which every row is padding (forward_xe would stop there)
    return d, Q, P, xv, xr


def repeated_inputs(name):
    """The same batch with every video repeated Q times: what xe_loss / forward_xe take."""
    d, Q, P, xv, xr = case_inputs(name)
    x = {k: np.repeat(a, Q, axis=0) for k, a in xv.items()}
    x.update(xr)
    return d._replace(B=d.B * Q), P, x


def composed(P, xv, xr, Q, d, train=True, p=0.0, seed=0, weight_class=WEIGHT_CLASS, cls=True, grad=True):
    """The composition of the module docstring.  P: {name: ndarray}.  Returns dict(loss, lm, cls, grads {name: ndarray} or None,
    running {name: tensor})."""
    Pt = xo.to_torch_params(P, requires_grad=grad)
    v, r = xo.to_torch_inputs(xv), xo.to_torch_inputs(xr)
    running = xo.new_running(d)
    with torch.set_grad_enabled(grad):
        V = xo.encoder_fwd(Pt, v["feats_rgb"], v["feats_opfl"], v["feat_mask"], train, p, seed, running)
        state = xo.init_hidden(Pt, V, v["feat_mask"])
        vproj = xo._lin(V, Pt, "lstmcore.v2a")
        rep = lambda t: t.repeat_interleave(Q, dim=0)      # noqa: E731
        Vr, vprojr = rep(V), rep(vproj)
        state = [(rep(h), rep(c)) for h, c in state]
        seq, mask = r["seq"], r["seq_mask"]
        outs, cats = [], []
        for i in range(seq.shape[1]):
            it = seq[:, i]
            out, state, _ = xo.core_step(Pt, Pt["embed.weight"][it], mask[:, i].unsqueeze(1), Vr, r["pos_feats"], state, p, seed, i,
                                         train, vprojr)
            logp, cat = xo.heads(Pt, out, p, seed, i, train)
            outs.append(logp)
            cats.append(cat)
        lm = xo.lm_criterion(torch.stack(outs, 1), seq, mask)
        lc = xo.cls_criterion(torch.stack(cats, 1), r["cap_classes"], mask, r["class_mask"]) if cls else torch.zeros(())
        loss = lm + (weight_class * lc if cls else 0.0)
        if grad:
            loss.backward()
    grads = None
    if grad:
        grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32)) for k, t in Pt.items()}
    return dict(loss=loss.item(), lm=lm.item(), cls=lc.item(), grads=grads, running=running)


@functools.lru_cache(maxsize=None)
def case_reference(name, train=True, p=0.0, seed=0):
    """composed() of a case (computed once per argument set, shared, never changed)."""
    d, Q, P, xv, xr = case_inputs(name)
    return composed(P, xv, xr, Q, d, train=train, p=p, seed=seed, cls=CASES[name][3], grad=train)


def repeated_reference(name):
    """xo.forward_xe + criteria + backward on the repeated batch at p = 0: dict as composed()."""
    dm, P, x = repeated_inputs(name)
    cls = CASES[name][3]
    Pt = xo.to_torch_params(P, requires_grad=True)
    xi = xo.to_torch_inputs(x)
    running = xo.new_running(dm)
    logp, cat, _ = xo.forward_xe(Pt, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"], xi["seq_mask"],
                                 train=True, running=running)
    lm = xo.lm_criterion(logp, xi["seq"], xi["seq_mask"])
    lc = xo.cls_criterion(cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"]) if cls else torch.zeros(())
    loss = lm + (WEIGHT_CLASS * lc if cls else 0.0)
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32)) for k, t in Pt.items()}
    return dict(loss=loss.item(), lm=lm.item(), cls=lc.item(), grads=grads, running=running)


# ---- what a case reaches (csrc/xg_train_video.hip launchers, csrc/xg_model.hip: step_packed)
def packed(c):
    return c["R"] % 8 == 0 and c["E"] % 4 == 0 and c["A"] % 4 == 0


def attn_bwd_group_form(c):
    """xgk_attn_bwd_group_form for aligned operands: the group kernel (True) or one workgroup per row (False)."""
    return c["A"] % 4 == 0 and c["R"] % 4 == 0 and 4 * GROUP * (c["R"] + (c["K"] + 3) // 4 * 4) <= 60000


def post_frame_parts(c, Q):
    """xgk_attn_post_dV_group: (workgroups a video's frames are dealt to, frames of each but the last, chunks of 16 (step, row) pairs)."""
    K, T = c["K"], c["L"] + 1
    n = max(min(Q, 16, K), -(-K // 512))
    kper = -(-K // n)
    return -(-K // kper), kper, -(-T * Q // 16)
