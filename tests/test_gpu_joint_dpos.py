"""The caption loss's gradient with respect to pos_feats on the MI355X (include/xgate_joint.h; docs/JOINT_TRAINING.md): what
SAModel.xe_loss, xe_loss_per_video, xe_loss_ss and xe_loss_ss_per_video return for a pos_feats that requires a gradient, against
float64 autograd of the existing oracle of each path with pos_feats as a leaf (tests/joint_oracle.py).

Bounds: tests/util.grad_misses at its defaults for every parameter gradient and for `dpos`, one more named entry.  dpos gets NO ReLU-flip
exemption (dt = dy (g + 1) crosses no ReLU derivative); the parameter gradients keep those of oracle_f64_with_flips.
Which kernel form ran is read from xgj_last_kernel_width(): four-wide at R = 24, scalar at R = 18 and for an output pointer that is not
16-byte aligned."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from tests import cap_ss_oracle as sso
from tests import joint_oracle as jo
from tests import ws_state
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, grad_misses, make_model, model_grads

pytestmark = pytest.mark.gpu

SCALE = 0.37                 # the non-unit dloss: the loss is multiplied by it before backward()
DROP_SEED = 24680

# kind -> (method, dims, Q, drop_prob_lm, scheduled sampling)
KINDS = {
    "xe": ("xe_loss", jo.CAP_TINY, 0, 0.0, False),
    "xe_drop": ("xe_loss", jo.CAP_TINY, 0, 0.5, False),
    "xe_x3": ("xe_loss", jo.CAP_TINY, 0, 0.0, False),            # precision "bf16x3" (split-bf16: the fp32 path's bounds)
    "xe_r18": ("xe_loss", jo.CAP_ODD, 0, 0.0, False),            # R % 4 != 0: the scalar kernel; nothing aligned, B = 3
    "xe_r18_drop": ("xe_loss", jo.CAP_ODD, 0, 0.5, False),
    "video_q3": ("xe_loss_per_video", jo.CAP_TINY, 3, 0.0, False),      # Q no multiple of the group of 4
    "video_q5": ("xe_loss_per_video", jo.CAP_TINY, 5, 0.0, False),
    "ss": ("xe_loss_ss", jo.CAP_TINY, 0, 0.0, True),             # tests/cap_ss_oracle.py "tiny": ss_prob 0.5, its uniforms
    "ss_video_q3": ("xe_loss_ss_per_video", jo.CAP_TINY, 3, 0.0, True),      # ... "v_tiny_q3"
}
FOUR_CALLS = ("xe", "video_q3", "ss", "ss_video_q3")
# What the existing kernels accumulate by float atomics, so that two identical runs of the SAME code differ in their last bits: the
# cross-entropy's row sums (xg_heads.hip: the loss), the embedding scatter-add (xg_pointwise.hip: embed.weight) and the attention's
# post pass (xg_attn.hip / xg_train_video.hip: lstmcore.a2w.weight).  Measured on an MI355X at these shapes between two runs without
# the request: loss 4.8e-7 to 9.5e-7 apart, these two gradients up to 4.7e-10 apart, every other gradient bit for bit.
ATOMIC_GRADS = ("embed.weight", "lstmcore.a2w.weight")
LOSS_ULPS = 5e-6             # tests/test_gpu_cap_ss.py: ten units in the last place of a float32 below 8
PRECISION = {"xe_x3": "bf16x3"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """(d, Q, P, x, uniforms or None): x holds the videos' features and the rows' pos_feats, seq, seq_mask, cap_classes, class_mask
    (row b Q + q).  numpy, made once, never changed."""
    method, cfg, Q, p, ss = KINDS[kind]
    if ss:
        d, Q_, P, x, u_sel, u_tok = sso.case_inputs("tiny" if Q == 0 else "v_tiny_q3")
        assert Q_ == Q and dict(d._asdict()) == dict(pg.make_dims(**cfg)._asdict())
        return d, Q, P, x, (u_sel, u_tok)
    d = pg.make_dims(**cfg)
    P = pg.make_params(d)
    v = pg.make_inputs(d, seed=3, ragged=True)
    M = d.B * max(Q, 1)
    r = v if Q == 0 else pg.make_inputs(d._replace(B=M), seed=4, ragged=True)
    x = {k: v[k] for k in ("feats_rgb", "feats_opfl", "feat_mask")}
    x.update({k: r[k].copy() for k in ("pos_feats", "seq", "seq_mask", "cap_classes", "class_mask")})
    if Q == 0:
        # the longest caption ends two steps short of T (the reference's loop would stop there; the device runs all T steps), and
        # row 1 is BOS only
        cut = d.L - 1
        x["seq"][:, cut:] = 0
        x["seq_mask"][:, cut:] = 0.0
        x["seq"][1, 1:] = 0
        x["seq_mask"][1, 1:] = 0.0
        assert x["seq_mask"][:, cut - 1].sum() > 0 and x["seq_mask"].sum(1).min() == 1.0
    return d, Q, P, x, None


def _device_args(kind, requires_grad):
    d, Q, P, x, _ = _inputs(kind)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    rows = lambda a: t(a) if Q == 0 else t(a).reshape(d.B, Q, *a.shape[1:])      # noqa: E731
    pos = rows(x["pos_feats"]).requires_grad_(requires_grad)
    return [t(x["feats_rgb"]), t(x["feats_opfl"]), t(x["feat_mask"]), pos, rows(x["seq"]), rows(x["seq_mask"]),
            rows(x["cap_classes"]), rows(x["class_mask"]), WEIGHT_CLASS]


def _model(kind, precision=None):
    method, cfg, Q, p, ss = KINDS[kind]
    d, _, P, _, u = _inputs(kind)
    m = make_model(d, P, p_drop=p, precision=precision or PRECISION.get(kind, "fp32"))
    if p > 0:
        m.dropout_seed = DROP_SEED
    if ss:
        m.ss_prob = 0.5
        m.ss_uniforms = (torch.from_numpy(u[0]).cuda(), torch.from_numpy(u[1]).cuda())
    return m


def _step(model, kind, requires_grad=True):
    """One call and (SCALE * loss).backward(): dict(loss, last_losses, grads, dpos or None, fed tokens or None, pos)."""
    from controllable_xgating_amd import _native_joint as nj
    model.zero_grad(set_to_none=True)
    args = _device_args(kind, requires_grad)
    loss = getattr(model, KINDS[kind][0])(*args)
    (loss * SCALE).backward()
    torch.cuda.synchronize()
    pos = args[3]
    tok = model.last_ss_tokens.cpu().numpy() if KINDS[kind][4] else None
    return dict(loss=loss.detach().clone(), ll=model.last_losses.clone(), grads={k: torch.from_numpy(v) for k, v in model_grads(model).items()},
                dpos=None if pos.grad is None else pos.grad.detach().clone(), tok=tok, width=nj.lib().xgj_last_kernel_width())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_dpos_and_every_parameter_gradient_against_float64_autograd(kind):
    method, cfg, Q, p, ss = KINDS[kind]
    d, _, P, x, _ = _inputs(kind)
    out = _step(_model(kind), kind)
    assert out["dpos"] is not None and tuple(out["dpos"].shape) == ((d.B, d.R) if Q == 0 else (d.B, Q, d.R))
    loss_o, g64, ex, dpos_o = jo.caption_reference(P, x, d, Q, True, p, DROP_SEED if p > 0 else 0, forced=out["tok"], scale=SCALE)
    print("%s: loss %.6f (oracle %.6f), max |dpos| %.3e (oracle %.3e), kernel width %d"
          % (kind, SCALE * float(out["loss"]), loss_o, float(out["dpos"].abs().max()), np.abs(dpos_o).max(), out["width"]))
    assert abs(SCALE * float(out["loss"]) - loss_o) < 1e-4
    assert np.abs(dpos_o).max() > 1e-4                      # (the reference really has a gradient there)
    got = {k: v.numpy() for k, v in out["grads"].items()}
    got["dpos"] = out["dpos"].reshape(-1, d.R).cpu().numpy()
    ref = dict(g64, dpos=dpos_o)
    assert "dpos" not in ex                                 # no ReLU-flip exemption for it
    report = {}
    bad = grad_misses(got, ref, skip=ZERO_GRAD_PARAMS, exempt=ex, report=report)
    print("%s: dpos (max error / scale, cosine, worst element / bound) %s" % (kind, report["dpos"][:3]))
    assert not bad, bad
    # which kernel form ran: the launcher's own word
    assert out["width"] == (4 if d.R % 4 == 0 else 1), (d.R, out["width"])
    if Q == 0 and not ss:
        # the BOS-only row still has a gradient (its step 0 counts), and it is the oracle's
        assert np.abs(dpos_o[1]).max() > 0


@pytest.mark.parametrize("kind", FOUR_CALLS)
def test_asking_for_dpos_changes_nothing_else_and_is_reproducible(kind):
    """Every parameter gradient with pos_feats.requires_grad True and False: bit for bit (the same launches, the sum runs behind them),
    except the two that the existing backward accumulates by float atomics (ATOMIC_GRADS), which two runs of the same code do not
    reproduce either: those by grad_misses at its defaults, the loss (atomic row sums) within ten units in the last place.  Two calls:
    bit-identical dpos."""
    model = _model(kind)
    a = _step(model, kind, True)
    b = _step(model, kind, False)
    c = _step(model, kind, True)
    assert b["dpos"] is None
    assert abs(float(a["loss"]) - float(b["loss"])) <= LOSS_ULPS and float((a["ll"] - b["ll"]).abs().max()) <= LOSS_ULPS
    if a["tok"] is not None:
        assert np.array_equal(a["tok"], b["tok"])
    diff = [n for n in a["grads"] if n not in ATOMIC_GRADS and not torch.equal(a["grads"][n], b["grads"][n])]
    assert not diff, diff
    bad = grad_misses({n: a["grads"][n].numpy() for n in ATOMIC_GRADS}, {n: b["grads"][n].numpy() for n in ATOMIC_GRADS})
    assert not bad, bad
    assert torch.equal(a["dpos"], c["dpos"])
    assert float(a["dpos"].abs().max()) > 0


class _Spy:
    """The binding with xgj_caption_dpos counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != "xgj_caption_dpos":
            return f

        def counted(*a):
            self.calls += 1
            return f(*a)
        return counted


def test_no_gradient_is_formed_when_nobody_asks(monkeypatch):
    """pos_feats without requires_grad, and a call under no_grad with one that has it: xgj_caption_dpos does not run."""
    from controllable_xgating_amd import _native_joint as nj
    spy = _Spy(nj.lib())
    monkeypatch.setattr(nj, "lib", lambda: spy)
    model = _model("xe")
    _step(model, "xe", False)
    with torch.no_grad():
        model.xe_loss(*_device_args("xe", True))
    assert spy.calls == 0
    out = _step(model, "xe", True)
    assert spy.calls == 1 and out["dpos"] is not None


def test_precision_bf16_refuses_a_pos_feats_that_requires_a_gradient():
    model = _model("xe", "bf16")
    with pytest.raises(NotImplementedError, match="gradient of pos_feats"):
        model.xe_loss(*_device_args("xe", True))
    model.ss_prob = 0.0
    with pytest.raises(NotImplementedError, match="gradient of pos_feats"):
        model.xe_loss_ss(*_device_args("xe", True))             # (ss_prob 0: it hands the call to xe_loss)
    model.xe_loss(*_device_args("xe", False)).backward()        # without the request the bf16 path runs as before
    with torch.no_grad():
        model.xe_loss(*_device_args("xe", True))                # ... and so it does where no gradient is recorded
    torch.cuda.synchronize()


# ---- the workspace
def _ranges(dims, Q, form):
    L = C.CDLL(__import__("controllable_xgating_amd")._native.LIB_DIAG_PATH)
    L.xgj_debug_ranges.restype = C.c_int
    out = (C.c_uint64 * 5)()
    assert L.xgj_debug_ranges(C.byref(dims), C.c_int32(Q), C.c_int32(form), out) == 0
    return [int(v) for v in out]


def _workspace_of(model, kind):
    """(XgDims, the 256-byte aligned workspace) the last call of `kind` ran in."""
    Q = KINDS[kind][2]
    if Q == 0:
        bufs = ws_state.pool_buffers(model)
        assert len(bufs) == 1
        return bufs[0]
    if KINDS[kind][4]:
        d = _inputs(kind)[0]
        return model._dims(d.B, d.K, d.L + 1), ws_state.aligned(model._last_ss_ws)
    dims, Q_, ws = model._last_video_ws
    assert Q_ == Q
    return dims, ws_state.aligned(ws)


def _direct_dpos(dims, Q, form, ws, n, misalign=False):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_joint as nj
    from controllable_xgating_amd.model import _stream
    buf = torch.full((n + 8,), float("nan"), device="cuda")
    out = buf[1:1 + n] if misalign else buf[:n]
    assert (out.data_ptr() % 16 != 0) == misalign
    x, run = nv.XgBatch(), nv.XgRun()
    nv.check(nj.lib().xgj_caption_dpos(_stream(), C.byref(dims), Q, form, C.byref(x), C.byref(run), ws.data_ptr(), ws.numel(),
                                       out.data_ptr()), "xgj_caption_dpos")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n + 1 if misalign else n:]).all()) and (not misalign or bool(torch.isnan(buf[:1]).all()))   # nothing past the ends
    return out.clone(), nj.lib().xgj_last_kernel_width()


@pytest.mark.parametrize("kind", FOUR_CALLS)
def test_dpos_reads_only_dposg_and_gp_and_the_workspace_stays_usable(kind):
    """Between the backward and xgj_caption_dpos every byte of the workspace but the two blocks the sum reads becomes NaN: the result
    is finite and bit for bit what the call returned.  The same through the scalar kernel (an output that is not 16-byte aligned).
    Afterwards the workspace, put back as the backward left it, serves the existing entry points as before."""
    from controllable_xgating_amd import _native_joint as nj
    method, cfg, Q, p, ss = KINDS[kind]
    form = nj.XGJ_FORM_SS if ss else (nj.XGJ_FORM_VIDEO if Q else nj.XGJ_FORM_XE)
    model = _model(kind)
    first = _step(model, kind)
    dims, ws = _workspace_of(model, kind)
    o_d, n_d, o_g, n_g, total = _ranges(dims, Q, form)
    assert ws.numel() >= total and o_d + n_d <= total and o_g + n_g <= total and (o_d + n_d <= o_g or o_g + n_g <= o_d)
    n = first["dpos"].numel()
    same, w4 = _direct_dpos(dims, Q, form, ws, n)
    assert w4 == 4 and torch.equal(same, first["dpos"].reshape(-1))          # the call formed again from the saved tensors
    snap = ws.clone()
    ws.fill_(255)                                                            # 0xFF bytes: every float a NaN
    ws[o_d:o_d + n_d] = snap[o_d:o_d + n_d]
    ws[o_g:o_g + n_g] = snap[o_g:o_g + n_g]
    poisoned, _ = _direct_dpos(dims, Q, form, ws, n)
    scalar, w1 = _direct_dpos(dims, Q, form, ws, n, misalign=True)
    ws.copy_(snap)
    assert bool(torch.isfinite(poisoned).all()) and torch.equal(poisoned, first["dpos"].reshape(-1))
    assert w1 == 1 and torch.equal(scalar, poisoned)
    # the existing entry points on the same workspace
    again = _step(model, kind)
    assert _workspace_of(model, kind)[1].data_ptr() == ws.data_ptr()
    assert abs(float(again["loss"]) - float(first["loss"])) <= 5e-6
    bad = grad_misses({k: v.numpy() for k, v in again["grads"].items()}, {k: v.numpy() for k, v in first["grads"].items()},
                      skip=ZERO_GRAD_PARAMS)
    assert not bad, bad
    if Q == 0 and not ss:
        from controllable_xgating_amd import LanguageModelCriterion
        a = _device_args(kind, False)
        model.zero_grad(set_to_none=True)
        logp, _ = model(*a[:6])
        LanguageModelCriterion()(logp, a[4], a[5]).backward()
        model.eval()
        with torch.no_grad():
            seq, _ = model.sample(a[0], a[1], a[2], a[3], {"sample_max": 1})
        torch.cuda.synchronize()
        assert all(np.isfinite(g).all() for g in model_grads(model).values()) and seq.shape[0] == a[0].shape[0]
