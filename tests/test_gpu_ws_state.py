"""No entry point may depend on what a workspace held before (include/xgate.h: zero-filled ONCE, then any call in any order).

Every other GPU test starts from a workspace that torch.zeros() just made.  Here each entry-point sequence runs twice with the
same inputs: on a freshly zeroed workspace, then on the same buffer after tests/ws_state.poison() (NaN in every data word, valid
but wrong tokens, the synchronisation words untouched) with every output buffer poisoned too.  A region that a call reads
without having written it -- an accumulator one of the two zeroing paths forgot, a bf16 mirror nobody refreshed, a stale value
under a zero mask -- then shows as a NaN or a wrong number.

Cells of (a) (sequence groups x configurations; every axis value meets every group at least once):

    groups   xe     : xg_forward_xe + xg_backward_xe;  xg_xe_loss_fwd + xg_xe_loss_bwd;  xg_forward_ss + xg_backward_ss
             roll   : xg_rollout GREEDY (no backward), SAMPLE and REPLAY (save = 1) + xg_rollout_bwd
             pair   : xg_rollout_pair + xg_rollout_compact, xg_rollout_pair_compact, xg_rollout_pair_videos(compact = 1), each
                      + xg_rollout_bwd on ws1; xg_rollout_pair_videos(compact = 0)
             blocks : xg_encoder_fwd + xg_encoder_bwd; xg_init_hidden; xg_vproj; xg_step_fwd (save = 1) + xg_step_bwd
             eval   : train = 0, save = 0 of xe and roll
    configs  A  tiny  gemm_mode 0                       aux NULL  packed NULL  drop_p 0
             B  odd   gemm_mode 1, mirror workspace     aux set   packed NULL  drop_p 0.5   (R % 8 != 0: the generic step path)
             C  mid   gemm_mode 1, mirror-less workspace aux NULL  packed set   drop_p 0.5
             D  mid   gemm_mode 3                       aux set   packed set   drop_p 0     (+ float64 oracle)
             E  mid   gemm_mode 0                       aux set   packed set   drop_p 0     (+ float64 oracle)
             F  mid   gemm_mode 1, mirror workspace     aux NULL  packed set   drop_p 0     (+ float64 oracle)
             P  c1    gemm_mode 0                       aux set   packed set   drop_p 0     (production size; group xe without forward_ss,
                                                                                             group pair: pair_videos(compact = 1) only)
    All inputs are the ragged ones (short captions: seq_mask rows of zeros; three videos with padded frames).
    The float64 oracle check (oracle_f64_with_flips + grad_misses) runs on the POISONED run of xg_xe_loss_fwd/bwd.
    Bit-wise cells: the in-place steps and the fp32 greedy rollout of test_gpu_parity.py, at their c1 sizes.
(b) every test above ends with sync_words_zero on every workspace it used; forwards without their backward have their own test.
(c) test_order_of_use_does_not_matter, (d) test_*accumulate* / test_criteria_*, (e) test_pool_*, (f) the negative control.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import ws_state as wss
from tests.util import CFG, WEIGHT_CLASS, ZERO_GRAD_PARAMS, grad_misses, make_model, oracle_f64_with_flips, to_dev

pytestmark = pytest.mark.gpu

INT_POISON = -7
CONFIGS = {
    "A": dict(tag="tiny", mode=0, aux=False, packed=False, drop_p=0.0),
    "B": dict(tag="odd", mode=1, aux=True, packed=False, drop_p=0.5),
    "C": dict(tag="mid", mode=1, ws_mode=0, aux=False, packed=True, drop_p=0.5),
    "D": dict(tag="mid", mode=3, aux=True, packed=True, drop_p=0.0),
    "E": dict(tag="mid", mode=0, aux=True, packed=True, drop_p=0.0),
    "F": dict(tag="mid", mode=1, aux=False, packed=True, drop_p=0.0),
    "P": dict(tag="c1", mode=0, aux=True, packed=True, drop_p=0.0),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


def _nv():
    from controllable_xgating_amd import _native as nv
    nv.lib()
    return nv


def _S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    nv = _nv()
    nv.check(getattr(nv.lib(), name)(*args), name)


def aux_handle():
    """The process-wide side-stream handle of the current stream (shared with the models: one handle per caller stream)."""
    from controllable_xgating_amd import model as M
    st = torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    if key not in M._AUX_HANDLES:
        out = C.c_void_p()
        call("xg_aux_create", C.byref(out))
        M._AUX_HANDLES[key] = out.value
    return M._AUX_HANDLES[key]


def nanf(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def seeded(name, shape, lo=-1.0, hi=1.0, seed=21):
    return torch.from_numpy(pg.uniform(name, shape, seed, lo, hi)).cuda()


class Rig:
    """Parameters, gradients, inputs, XgRun and workspaces of one configuration, driven raw through ctypes."""

    def __init__(self, tag, mode=0, ws_mode=None, aux=False, packed=False, drop_p=0.0, **over):
        nv = self.nv = _nv()
        self.d = d = pg.make_dims(**dict(CFG[tag], **over))
        self.mode, self.ws_mode, self.drop_p = mode, (mode if ws_mode is None else ws_mode), drop_p
        self.Pn = pg.make_params(d)
        self.off, n = {}, 0
        for name in nv.PARAM_NAMES:
            self.off[name] = (n, self.Pn[name].size)
            n += (self.Pn[name].size + 63) // 64 * 64
        self.flat = torch.zeros(n, device="cuda")
        for name, (o, k) in self.off.items():
            self.flat[o:o + k].copy_(torch.from_numpy(self.Pn[name]).reshape(-1))
        self.g = torch.zeros(n, device="cuda")
        self.ps, self.gs = self._struct(self.flat), self._struct(self.g)
        self.xn = pg.make_inputs(d, seed=0, ragged=True)
        self.x = to_dev(self.xn)
        self.x2 = {k: torch.cat([v, v], 0).contiguous() for k, v in self.x.items()}
        self.T = d.L + 1
        self.aux = aux_handle() if aux else None
        self.packed_dtype, self.packed = {0: 0, 1: 1, 3: 2}[mode], None
        if packed:
            d1 = self.dims(1, 1)
            nb = nv.lib().xg_packed_bytes(C.byref(d1), self.packed_dtype)
            assert nb > 0, "this shape has no packed form"
            self._packed = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
            self.packed = (self._packed.data_ptr() + 15) & ~15
            call("xg_pack_weights", _S(), C.byref(d1), C.byref(self.ps), C.c_void_p(self.packed), C.c_size_t(nb), self.packed_dtype, 1)
        self._ws = {}
        self.g_start, self.keep_grads = None, False           # (d): what a backward finds in g (default: zeros)

    def start_grads(self):
        if self.keep_grads:
            return
        if self.g_start is None:
            self.g.zero_()
        else:
            self.g.copy_(self.g_start)

    def _struct(self, flat):
        s = self.nv.XgParams()
        for i, name in enumerate(self.nv.PARAM_NAMES):
            setattr(s, "p%d" % i, flat.data_ptr() + 4 * self.off[name][0])
        return s

    def grads(self, flat=None):
        flat = (self.g if flat is None else flat).detach().cpu().numpy()
        return {name: flat[o:o + k].reshape(self.Pn[name].shape) for name, (o, k) in self.off.items()}

    def dims(self, B=None, T=None):
        d = self.d
        return wss.make_xgdims(B or d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H, d.F1, d.F2, T or self.T)

    def ws(self, name, dims, zero_init=False):
        """(pointer, size) of the named workspace for `dims`; allocated zero-filled at first use, kept afterwards."""
        nbytes = self.nv.lib().xg_workspace_bytes_mode(C.byref(dims), self.ws_mode)
        if name not in self._ws:
            self._ws[name] = [torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda"), dims]
        buf = self._ws[name][0]
        assert buf.numel() >= nbytes + 256
        self._ws[name][1] = dims
        view = wss.aligned(buf)
        if zero_init:
            call("xg_workspace_init", _S(), C.c_void_p(view.data_ptr()), C.c_size_t(view.numel()))
        return C.c_void_p(view.data_ptr()), C.c_size_t(nbytes)

    def drop_workspaces(self):
        self._ws = {}

    def poison_all(self):
        torch.cuda.synchronize()
        for buf, dims in self._ws.values():
            wss.poison(wss.aligned(buf), dims, self.ws_mode)

    def sync_zero(self):
        torch.cuda.synchronize()
        return all(wss.sync_words_zero(wss.aligned(buf), dims, self.ws_mode) for buf, dims in self._ws.values())

    def run(self, save, train=1):
        r = self.nv.XgRun()
        r.train, r.drop_p, r.seed, r.save = train, self.drop_p, 0x51F15EED, save
        r.bn_momentum, r.bn_eps, r.gemm_mode, r.packed_dtype = 0.1, 1e-5, self.mode, self.packed_dtype
        r.packed, r.aux = self.packed, self.aux
        return r

    def bn(self):
        R = self.d.R
        t = torch.cat([torch.zeros(R), torch.ones(R), torch.zeros(R), torch.ones(R)]).cuda()
        s = self.nv.XgBnState()
        s.rgb_mean, s.rgb_var, s.opfl_mean, s.opfl_var = (t.data_ptr() + 4 * R * i for i in range(4))
        return s, t

    def batch(self, x=None, seq=True):
        x = self.x if x is None else x
        b = self.nv.XgBatch()
        b.feats_rgb, b.feats_opfl, b.feat_mask, b.pos_feats = (x[k].data_ptr() for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats"))
        if seq:
            b.seq, b.seq_mask = x["seq"].data_ptr(), x["seq_mask"].data_ptr()
        return b


# ---------------------------------------------------------------------------------------------------- the sequences
def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def seq_xe(r, train=1, save=1):
    d, x = r.dims(), r.x
    B, T = d.B, d.T
    wp, wn = r.ws("ws1", d)
    logp, cat = nanf(B, T, d.V), nanf(B, T, d.C)
    bn, bnt = r.bn()
    run, b = r.run(save, train), r.batch()
    call("xg_forward_xe", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), wp, wn, ptr(logp), ptr(cat))
    out = dict(logp=logp, cat_logp=cat, bn=bnt)
    if save:
        r.start_grads()
        dl, dc = seeded("dlogp", (B, T, d.V)) / (B * T), seeded("dcat", (B, T, d.C)) / (B * T)
        call("xg_backward_xe", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), C.byref(run), wp, wn, ptr(dl), ptr(dc))
        out["g"] = r.g
    return {k: v.clone() for k, v in out.items()}


def seq_xe_loss(r, train=1, save=1):
    d, x = r.dims(), r.x
    wp, wn = r.ws("ws1", d)
    losses = nanf(3)
    bn, bnt = r.bn()
    run, b = r.run(save, train), r.batch()
    call("xg_xe_loss_fwd", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), ptr(x["cap_classes"]), ptr(x["class_mask"]),
         WEIGHT_CLASS, C.byref(run), wp, wn, ptr(losses))
    out = dict(loss=losses, bn=bnt)
    if save:
        r.start_grads()
        call("xg_xe_loss_bwd", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), ptr(x["cap_classes"]), ptr(x["class_mask"]),
             WEIGHT_CLASS, None, C.byref(run), wp, wn)
        out["g"] = r.g
    return {k: v.clone() for k, v in out.items()}


def seq_ss(r, train=1, save=1):
    d = r.dims()
    B, T = d.B, d.T
    wp, wn = r.ws("ws1", d)
    logp, cat = nanf(B, T, d.V), nanf(B, T, d.C)
    u_sel, u_tok = seeded("u_sel", (T, B), 0.0, 1.0), seeded("u_tok", (T, B), 0.0, 1.0)
    bn, bnt = r.bn()
    run, b = r.run(save, train), r.batch()
    call("xg_forward_ss", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), 0.25, ptr(u_sel), ptr(u_tok), wp, wn,
         ptr(logp), ptr(cat))
    out = dict(logp=logp, cat_logp=cat, bn=bnt)
    if save:
        r.start_grads()
        dl, dc = seeded("dlogp", (B, T, d.V)) / (B * T), seeded("dcat", (B, T, d.C)) / (B * T)
        call("xg_backward_ss", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), C.byref(run), wp, wn, ptr(dl), ptr(dc))
        out["g"] = r.g
    return {k: v.clone() for k, v in out.items()}


def _rollout_outputs(B, T, parts):
    return (torch.full((B, T - 1), INT_POISON, dtype=torch.int64, device="cuda"), nanf(B, T - 1),
            torch.full((parts,), INT_POISON, dtype=torch.int32, device="cuda"))


def _check_tail(seq, n, rows=slice(None)):
    """include/xgate.h: columns past the reference's early exit are zero tokens (written by the library, not by the caller)."""
    assert bool((seq[rows, int(n):] == 0).all()), (int(n), seq[rows].tolist())


def seq_rollout(r, mode, train=1, save=1, backward=True):
    nv = r.nv
    d = r.dims()
    B, T = d.B, d.T
    wp, wn = r.ws("ws1", d)
    seq, slp, n = _rollout_outputs(B, T, 1)
    uni = seeded("uni", (T, B), 0.0, 1.0) if mode == nv.XG_ROLLOUT_SAMPLE else None
    forced = r.x["seq"][:, 1:].contiguous() if mode == nv.XG_ROLLOUT_REPLAY else None
    bn, bnt = r.bn()
    run, b = r.run(save, train), r.batch(seq=False)
    call("xg_rollout", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), mode, ptr(uni), ptr(forced), 1.0, wp, wn,
         ptr(seq), ptr(slp), ptr(n))
    out = dict(seq=seq, seq_logp=slp, n_steps=n, bn=bnt)
    if save and backward:
        r.start_grads()
        ds = seeded("dslp", (B, T - 1)) / B
        call("xg_rollout_bwd", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), C.byref(run), wp, wn, ptr(ds))
        out["g"] = r.g
    out = {k: v.clone() for k, v in out.items()}
    if mode != nv.XG_ROLLOUT_REPLAY:
        torch.cuda.synchronize()
        _check_tail(out["seq"], out["n_steps"][0])
    return out


def seq_pair(r, kind, train=1, save=1):
    """kind: 'pair' (+ xg_rollout_compact), 'pair_compact', 'videos1', 'videos0' (no backward)."""
    d1, d2 = r.dims(), r.dims(B=2 * r.d.B)
    B, T = d1.B, d1.T
    wp2, wn2 = r.ws("ws2", d2)
    wp1, wn1 = r.ws("ws1", d1)
    seq, slp, n = _rollout_outputs(2 * B, T, 2)
    uni = seeded("uni", (T, B), 0.0, 1.0)
    bn, bnt = r.bn()
    run, b1, b2 = r.run(save, train), r.batch(seq=False), r.batch(r.x2, seq=False)
    common = (_S(), C.byref(d2), C.byref(r.ps), C.byref(bn))
    if kind == "pair":
        call("xg_rollout_pair", *common, C.byref(b2), C.byref(run), B, ptr(uni), 1.0, wp2, wn2, ptr(seq), ptr(slp), ptr(n))
        call("xg_rollout_compact", _S(), C.byref(d2), wp2, wn2, C.byref(d1), wp1, wn1)
    elif kind == "pair_compact":
        call("xg_rollout_pair_compact", *common, C.byref(b2), C.byref(run), B, ptr(uni), 1.0, wp2, wn2, C.byref(d1), wp1, wn1,
             ptr(seq), ptr(slp), ptr(n))
    else:
        call("xg_rollout_pair_videos", *common, C.byref(b1), C.byref(run), ptr(uni), 1.0, wp2, wn2, C.byref(d1), wp1, wn1,
             1 if kind == "videos1" else 0, ptr(seq), ptr(slp), ptr(n))
    out = dict(seq=seq, seq_logp=slp, n_steps=n, bn=bnt)
    if save and kind != "videos0":
        r.start_grads()
        ds = seeded("dslp", (B, T - 1)) / B
        call("xg_rollout_bwd", _S(), C.byref(d1), C.byref(r.ps), C.byref(r.gs), C.byref(b1), C.byref(run), wp1, wn1, ptr(ds))
        out["g"] = r.g
    out = {k: v.clone() for k, v in out.items()}
    torch.cuda.synchronize()
    _check_tail(out["seq"], out["n_steps"][0], slice(0, B))
    _check_tail(out["seq"], out["n_steps"][1], slice(B, 2 * B))
    return out


def seq_blocks(r, train=1, step_backward=True, dacc=None, null_optional=False):
    """The building blocks: encoder forward / backward, init_hidden, v2a(V), one raw step forward / backward with a held row.
    dacc: optional (dV, dvproj, dpos) start values of the step backward's accumulated outputs (default zeros)."""
    d = r.dims()
    B, K, R, A = d.B, d.K, d.R, d.A
    wp, wn = r.ws("ws1", d)
    V, state, vproj = nanf(B, K, R), nanf(4, B, R), nanf(B, K, A)
    bn, bnt = r.bn()
    run, b = r.run(1, train), r.batch()
    call("xg_encoder_fwd", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), wp, wn, ptr(V))
    r.start_grads()
    dVenc = seeded("dVenc", (B, K, R))
    call("xg_encoder_bwd", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), C.byref(run), wp, wn, ptr(dVenc))
    out = dict(V=V, bn=bnt, g_enc=r.g.clone())
    call("xg_init_hidden", _S(), C.byref(d), C.byref(r.ps), ptr(V), ptr(r.x["feat_mask"]), wp, wn, ptr(state))
    call("xg_vproj", _S(), C.byref(d), C.byref(r.ps), ptr(V), ptr(vproj), C.byref(run))
    out.update(state0=state.clone(), vproj=vproj)
    tok = r.x["seq"][:, 1].contiguous()
    mk = r.x["seq_mask"][:, -1].contiguous()                 # ragged: the short captions' rows are held
    assert 0 < float(mk.sum()) < B
    logp, alpha = nanf(B, d.V), nanf(B, K)
    call("xg_step_fwd", _S(), C.byref(d), C.byref(r.ps), ptr(tok), ptr(mk), ptr(V), ptr(vproj), ptr(r.x["pos_feats"]), C.byref(run), 2,
         wp, wn, ptr(state), ptr(logp), ptr(alpha))
    out.update(state1=state, step_logp=logp, alpha=alpha)
    if step_backward:
        r.start_grads()
        dnew, dstate = seeded("dstate_new", (4, B, R)), nanf(4, B, R)
        dV, dvp, dpos = (torch.zeros(B, K, R, device="cuda"), torch.zeros(B, K, A, device="cuda"), torch.zeros(B, R, device="cuda")) \
            if dacc is None else [t.clone() for t in dacc]
        if null_optional:
            dV = dvp = dpos = None
        call("xg_step_bwd", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), ptr(tok), ptr(mk), ptr(V), ptr(vproj), ptr(r.x["pos_feats"]),
             C.byref(run), 2, wp, wn, ptr(state), ptr(dnew), ptr(dstate), ptr(dV), ptr(dvp), ptr(dpos))
        out.update(dstate=dstate, g_step=r.g)
        if not null_optional:
            out.update(dV=dV, dvproj=dvp, dpos=dpos)
    return {k: v.clone() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- comparisons
def same_as(a, b, what, exact=()):
    """Outputs `b` of a run against those of the reference run `a`: nothing non-finite, no poison left, integers equal, floats
    within the suite's bound for two runs of the same call (test_repeated_iterations_are_reproducible_across_streams) -- or
    bit for bit where `exact` names them."""
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        ta, tb = a[k].cpu(), b[k].cpu()
        for t in (ta, tb):
            if t.is_floating_point():
                assert bool(torch.isfinite(t).all()), (what, k, "non-finite / unwritten", int((~torch.isfinite(t)).sum()), t.numel())
            else:
                assert not bool((t == INT_POISON).any()), (what, k, "unwritten")
        if not ta.is_floating_point() or k in exact:
            assert torch.equal(ta, tb), (what, k, "differs")
        elif k == "loss":
            for la, lb in zip(ta.tolist(), tb.tolist()):
                assert abs(la - lb) <= 5e-6 * max(1.0, abs(la)), (what, k, la, lb)
        else:
            err, scale = float((ta.double() - tb.double()).abs().max()), float(ta.abs().max())
            print("%-40s %-10s max|a-b| %.3e  max|a| %.3e" % (what, k, err, scale))
            assert err <= 1e-5 * scale + 1e-8, (what, k, err, scale)


def fresh_vs_poisoned(r, fn, what, exact=()):
    """fn(r) on freshly zeroed workspaces, then on the same buffers poisoned; the synchronisation words are zero after each."""
    r.drop_workspaces()
    a = fn(r)
    assert r.sync_zero(), (what, "fresh")
    r.poison_all()
    b = fn(r)
    assert r.sync_zero(), (what, "poisoned")
    same_as(a, b, what, exact)
    return a, b


@functools.lru_cache(maxsize=None)
def _oracle_xe_mid():
    d = pg.make_dims(**CFG["mid"])
    Pn, xn = pg.make_params(d), pg.make_inputs(d, seed=0, ragged=True)

    def fn(P, xi, tr):
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"], xi["seq_mask"],
                                     train=True, running=xo.new_running(d), relu_trace=tr)
        l_xe = xo.lm_criterion(logp, xi["seq"], xi["seq_mask"])
        l_cls = xo.cls_criterion(cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"])
        return l_xe + WEIGHT_CLASS * l_cls, None
    loss, _, g64, ex = oracle_f64_with_flips(Pn, xn, fn)
    return loss, g64, ex


def bf16_misses(grads, ref, exempt):
    """The bf16 bounds of test_config5_b128_hidden1024_bf16_and_split_bf16_vs_oracle (norm 5 %, cosine 0.999 / 0.997 in front of
    BatchNorm, elements 3 % / 6 % / 12 % of the largest one), over every element that no ReLU flip may move."""
    bad = []
    for name, g in grads.items():
        if name in ZERO_GRAD_PARAMS:
            continue
        r = ref[name]
        scale = float(np.abs(r).max())
        keep = np.ones(r.shape, bool) if name not in exempt else ~exempt[name]
        gd, rd = np.asarray(g, np.float64)[keep], np.asarray(r, np.float64)[keep]
        gn, rn = np.linalg.norm(gd), np.linalg.norm(rd)
        if not abs(gn - rn) <= 5e-2 * rn + 1e-6:
            bad.append((name, "norm", gn, rn))
        pre_bn = name in ("two_spatial_encoder.visual_emb_rgb.0.weight", "two_spatial_encoder.visual_emb_opfl.0.weight")
        cos = float(gd @ rd) / max(gn * rn, 1e-300)
        if rn > 1e-9 and not cos >= (0.997 if pre_bn else 0.999):
            bad.append((name, "cosine", cos))
        tol_e = (1.2e-1 if name == "lstmcore.gate.gate.0.bias" else (6e-2 if pre_bn else 3e-2)) * scale + 1e-7
        if gd.size and float(np.abs(gd - rd).max()) > tol_e:
            bad.append((name, "elements", float(np.abs(gd - rd).max()), tol_e))
    return bad


def check_poisoned_xe_loss_vs_oracle(r, out):
    loss_o, g64, ex = _oracle_xe_mid()
    loss, grads = float(out["loss"][0]), r.grads(out["g"])
    print("poisoned xe_loss, gemm_mode %d: loss %.7f oracle %.7f" % (r.mode, loss, loss_o))
    if r.mode == 1:
        assert abs(loss - loss_o) < 1e-2, (loss, loss_o)
        bad = bf16_misses(grads, g64, ex)
    else:
        assert abs(loss - loss_o) < 1e-4, (loss, loss_o)
        bad = grad_misses(grads, g64, skip=ZERO_GRAD_PARAMS, exempt=ex)
    assert not bad, (r.mode, bad)


# ---------------------------------------------------------------------------------------------------- (a) + (b)
@pytest.mark.parametrize("cfg", ["A", "B", "C", "D", "E", "F", "P"])
def test_poisoned_workspace_xe(cfg):
    r = Rig(**CONFIGS[cfg])
    fresh_vs_poisoned(r, seq_xe, cfg + " forward_xe+backward_xe")
    _, b = fresh_vs_poisoned(r, seq_xe_loss, cfg + " xe_loss_fwd+bwd")
    if cfg in ("D", "E", "F"):
        check_poisoned_xe_loss_vs_oracle(r, b)
    if cfg != "P":
        fresh_vs_poisoned(r, seq_ss, cfg + " forward_ss+backward_ss")


@pytest.mark.parametrize("cfg", ["A", "B", "C", "D", "E", "F"])
def test_poisoned_workspace_rollouts(cfg):
    r = Rig(**CONFIGS[cfg])
    nv = r.nv
    fresh_vs_poisoned(r, lambda q: seq_rollout(q, nv.XG_ROLLOUT_GREEDY, save=0), cfg + " rollout greedy")
    fresh_vs_poisoned(r, lambda q: seq_rollout(q, nv.XG_ROLLOUT_SAMPLE), cfg + " rollout sample+bwd")
    fresh_vs_poisoned(r, lambda q: seq_rollout(q, nv.XG_ROLLOUT_REPLAY), cfg + " rollout replay+bwd")


@pytest.mark.parametrize("cfg", ["A", "B", "C", "D", "E", "F", "P"])
def test_poisoned_workspace_rollout_pairs(cfg):
    r = Rig(**CONFIGS[cfg])
    for kind in (("videos1",) if cfg == "P" else ("pair", "pair_compact", "videos1", "videos0")):
        fresh_vs_poisoned(r, lambda q: seq_pair(q, kind), cfg + " " + kind)


@pytest.mark.parametrize("cfg", ["A", "B", "C", "D", "E", "F"])
def test_poisoned_workspace_building_blocks(cfg):
    r = Rig(**CONFIGS[cfg])
    fresh_vs_poisoned(r, seq_blocks, cfg + " encoder/init_hidden/vproj/step")


@pytest.mark.parametrize("cfg", ["A", "B", "C", "D", "E", "F"])
def test_poisoned_workspace_eval_mode(cfg):
    r = Rig(**CONFIGS[cfg])
    nv = r.nv
    fresh_vs_poisoned(r, lambda q: seq_xe(q, train=0, save=0), cfg + " eval forward_xe")
    fresh_vs_poisoned(r, lambda q: seq_xe_loss(q, train=0, save=0), cfg + " eval xe_loss_fwd")
    fresh_vs_poisoned(r, lambda q: seq_ss(q, train=0, save=0), cfg + " eval forward_ss")
    for mode in (nv.XG_ROLLOUT_GREEDY, nv.XG_ROLLOUT_SAMPLE, nv.XG_ROLLOUT_REPLAY):
        fresh_vs_poisoned(r, lambda q: seq_rollout(q, mode, train=0, save=0), cfg + " eval rollout %d" % mode)


@pytest.mark.parametrize("precision,rows", [("fp32", 128), ("bf16x3", 128), ("bf16", 128)])
def test_in_place_steps_are_bitwise_equal_on_a_poisoned_workspace(precision, rows):
    """The case of test_in_place_steps_are_bitwise_reproducible (three xg_step_fwd calls on an in-place state, c1 at 128 rows):
    the same bits on the pool's scratch workspace as it is and after poison()."""
    from controllable_xgating_amd.model import _ws_ptr
    d = pg.make_dims(**dict(CFG["c1"], B=rows))
    x = to_dev(pg.make_inputs(d, seed=0))
    model = make_model(d, train=False, precision=precision)
    with torch.no_grad():
        V = model.encode(x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
        st = model.init_hidden(V, x["feat_mask"])
        state0 = torch.cat([st[0][0], st[0][1], st[1][0], st[1][1]], 0).contiguous()
        dd = model._dims(d.B, d.K, 1)
        ps, run = model._params_struct(), model._run(False)
        vproj = torch.empty(d.B, d.K, model.att_size, device="cuda")
        call("xg_vproj", _S(), C.byref(dd), C.byref(ps), ptr(V), ptr(vproj), C.byref(run))
        wp, wn = _ws_ptr(model._pool.shared(dd, V.device))
        tok = x["seq"][:, 1].contiguous()
        first = None
        for rep in range(3):
            s = state0.clone()
            for _ in range(3):
                call("xg_step_fwd", _S(), C.byref(dd), C.byref(ps), ptr(tok), None, ptr(V), ptr(vproj), ptr(x["pos_feats"]), C.byref(run), 0,
                     wp, wn, ptr(s), None, None)
            torch.cuda.synchronize()
            assert wss.pool_sync_words_zero(model)
            assert bool(torch.isfinite(s).all())
            if first is None:
                first = s.clone()
            else:
                assert torch.equal(s, first), (precision, rows, rep, float((s - first).abs().max()))
            assert wss.poison_pool(model) >= 1


def test_greedy_rollout_is_bitwise_equal_on_a_poisoned_pool():
    """The fp32 case of test_greedy_rollout_is_reproducible (c1, 64 rows): identical tokens and log-probabilities with the
    pool's workspaces poisoned between the rollouts."""
    d = pg.make_dims(**dict(CFG["c1"], B=64))
    x = to_dev(pg.make_inputs(d, seed=0))
    model = make_model(d, train=False, precision="fp32")
    first = None
    for rep in range(3):
        with torch.no_grad():
            seq, lp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
        torch.cuda.synchronize()
        assert wss.pool_sync_words_zero(model) and bool(torch.isfinite(lp).all())
        if first is None:
            first = (seq.clone(), lp.clone())
        else:
            assert torch.equal(seq, first[0]) and torch.equal(lp, first[1]), rep
        assert wss.poison_pool(model) >= 1


@pytest.mark.parametrize("cfg", ["A", "C", "E"])
def test_forwards_without_their_backward_leave_the_sync_words_zero(cfg):
    """(b) A save = 1 forward that is never followed up, and xg_step_fwd alone: tickets and dsync are zero afterwards, and the next
    call on the workspace (poisoned in between) is as good as on a fresh one."""
    r = Rig(**CONFIGS[cfg])
    nv = r.nv
    ref = seq_xe_loss(r)
    r.drop_workspaces()
    for what, fn in (("forward_xe", lambda: _forward_only(r, "xe")),
                     ("xe_loss_fwd", lambda: _forward_only(r, "xe_loss")),
                     ("rollout sample", lambda: seq_rollout(r, nv.XG_ROLLOUT_SAMPLE, backward=False)),
                     ("pair videos", lambda: _forward_only(r, "videos")),
                     ("step_fwd", lambda: seq_blocks(r, step_backward=False))):
        fn()
        assert r.sync_zero(), what
        r.poison_all()
    same_as(ref, seq_xe_loss(r), cfg + " xe_loss after abandoned forwards")
    assert r.sync_zero()


def _forward_only(r, which):
    d, x = r.dims(), r.x
    wp, wn = r.ws("ws1", d)
    bn, _ = r.bn()
    run, b = r.run(1), r.batch()
    if which == "xe":
        logp, cat = nanf(d.B, d.T, d.V), nanf(d.B, d.T, d.C)
        call("xg_forward_xe", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), wp, wn, ptr(logp), ptr(cat))
    elif which == "xe_loss":
        losses = nanf(3)
        call("xg_xe_loss_fwd", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), ptr(x["cap_classes"]), ptr(x["class_mask"]),
             WEIGHT_CLASS, C.byref(run), wp, wn, ptr(losses))
    else:
        d2 = r.dims(B=2 * d.B)
        wp2, wn2 = r.ws("ws2", d2)
        seq, slp, n = _rollout_outputs(2 * d.B, d.T, 2)
        uni = seeded("uni", (d.T, d.B), 0.0, 1.0)
        call("xg_rollout_pair_videos", _S(), C.byref(d2), C.byref(r.ps), C.byref(bn), C.byref(r.batch(seq=False)), C.byref(run), ptr(uni), 1.0,
             wp2, wn2, C.byref(d), wp, wn, 1, ptr(seq), ptr(slp), ptr(n))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("cfg", ["C", "E"])
def test_order_of_use_does_not_matter(cfg):
    """One pair of workspaces, one XgDims, never re-initialised: rollout pair (save) + backward -> XE forward / backward -> raw
    xg_step_fwd -> eval rollout -> XE again; each stage equals the same stage alone on a fresh workspace.  Then the last batch of
    an epoch -- smaller B and T, another layout -- on the SAME allocation after xg_workspace_init, as the contract requires."""
    nv = _nv()
    stages = [("pair", lambda q: seq_pair(q, "videos1")), ("xe", seq_xe_loss), ("step", lambda q: seq_blocks(q, step_backward=False)),
              ("eval rollout", lambda q: seq_rollout(q, nv.XG_ROLLOUT_GREEDY, train=0, save=0)), ("xe again", seq_xe_loss)]
    alone = []
    for _, fn in stages:
        alone.append(fn(Rig(**CONFIGS[cfg])))
    r = Rig(**CONFIGS[cfg])
    for (what, fn), ref in zip(stages, alone):
        same_as(ref, fn(r), "%s in sequence: %s" % (cfg, what))
        assert r.sync_zero(), what
    # ---- other dims on the same allocation
    small = dict(B=r.d.B - 2, L=r.d.L - 3)
    ref = seq_xe_loss(Rig(**dict(CONFIGS[cfg], **small)))
    ref_roll = seq_rollout(Rig(**dict(CONFIGS[cfg], **small)), nv.XG_ROLLOUT_SAMPLE)
    q = Rig(**dict(CONFIGS[cfg], **small))
    q._ws = {"ws1": [r._ws["ws1"][0], q.dims()]}
    q.ws("ws1", q.dims(), zero_init=True)
    same_as(ref, seq_xe_loss(q), cfg + " smaller dims on the re-initialised allocation: xe")
    same_as(ref_roll, seq_rollout(q, nv.XG_ROLLOUT_SAMPLE), cfg + " smaller dims on the re-initialised allocation: rollout")
    assert q.sync_zero()


# ---------------------------------------------------------------------------------------------------- (d)
def _g0_like(scale, n):
    """A seeded start value of the gradient buffer: no element zero, of the gradient's own size."""
    u = seeded("g0", (n,), 0.5, 1.5) * torch.where(seeded("g0s", (n,)) < 0, -1.0, 1.0)
    return (u * scale).contiguous()


BACKWARDS = {
    "xe": (seq_xe, ("g",)), "xe_loss": (seq_xe_loss, ("g",)), "ss": (seq_ss, ("g",)),
    "rollout": (lambda r: seq_rollout(r, r.nv.XG_ROLLOUT_SAMPLE), ("g",)),
    "pair": (lambda r: seq_pair(r, "videos1"), ("g",)),
    "blocks": (seq_blocks, ("g_enc", "g_step")),              # xg_encoder_bwd and xg_step_bwd
}


@pytest.mark.parametrize("which", sorted(BACKWARDS))
@pytest.mark.parametrize("cfg", ["A", "E"])
def test_parameter_gradients_are_accumulated(cfg, which):
    """'Parameter gradients are ACCUMULATED into g': with g = g0 on entry every backward leaves g0 + grad (g - g0 against the
    zero-g run), and two passes without clearing leave 2 * grad."""
    fn, keys = BACKWARDS[which]
    r = Rig(**CONFIGS[cfg])
    base = fn(r)
    grads = {k: base[k].double().cpu() for k in keys}
    total = sum(grads.values())
    scales = {k: float(v.abs().max()) for k, v in grads.items()}
    assert min(scales.values()) > 0, scales

    def check(got, want, what):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print("%s %s %s: err %.3e scale %.3e" % (cfg, which, what, err, scale))
        assert bool(torch.isfinite(got).all()) and err <= 1e-5 * scale + 1e-8, (cfg, which, what, err, scale)
    r.g_start = _g0_like(min(scales.values()), r.g.numel())
    out = fn(r)
    for k in keys:
        check(out[k].double().cpu() - r.g_start.double().cpu(), grads[k], k + " - g0")
    r.g_start = None
    r.g.zero_()
    r.keep_grads = True
    fn(r)
    fn(r)
    torch.cuda.synchronize()
    check(r.g.double().cpu(), 2 * total, "two passes")


def test_step_backward_accumulates_optional_outputs_and_overwrites_dstate():
    r = Rig(**CONFIGS["E"])
    d = r.dims()
    base = seq_blocks(r)
    acc0 = (seeded("a.dV", (d.B, d.K, d.R)), seeded("a.dvp", (d.B, d.K, d.A)), seeded("a.dpos", (d.B, d.R)))
    acc = seq_blocks(r, dacc=acc0)
    for k, a0 in zip(("dV", "dvproj", "dpos"), acc0):
        scale = float(base[k].abs().max())
        assert scale > 0, k
        err = float((acc[k].double() - a0.double() - base[k].double()).abs().max())
        assert err <= 1e-5 * max(scale, float(a0.abs().max())) + 1e-8, (k, err, scale)
    same_as({"dstate": base["dstate"]}, {"dstate": acc["dstate"]}, "dstate (poisoned on entry: overwritten)")
    null = seq_blocks(r, null_optional=True)                          # NULL optional outputs are accepted
    same_as({k: base[k] for k in ("dstate", "g_step")}, {k: null[k] for k in ("dstate", "g_step")}, "step_bwd with NULL dV/dvproj/dpos")


@pytest.mark.parametrize("roll", [0, 1])
@pytest.mark.parametrize("with_mask2", [False, True])
def test_criteria_nll_backward_overwrites_dlogp(roll, with_mask2):
    """xg_nll_bwd: 'dlogp is OVERWRITTEN' -- every element of a NaN-filled dlogp, against the float64 formula
    -scale * scale_dev * mask * mask2 / sum(mask * mask2) at the (rolled) target, zero elsewhere.  Row 1 of the mask is all zero.
    Bound: the kernel forms each element with three fp32 roundings (two products, one quotient) of operands that are exact in
    fp32 except sum(mask), an exact integer: 4 ulp = 4 * 2^-24 relative."""
    B, T, V = 5, 7, 23
    tgt = torch.from_numpy(pg.randint("nll.t", (B, T), 3, 0, V)).cuda()
    mask = (seeded("nll.m", (B, T), 0.0, 1.0) < 0.7).float()
    mask[1] = 0.0
    mask[0, 0] = 1.0
    m2 = (seeded("nll.m2", (B, T), 0.0, 1.0) < 0.8).float() if with_mask2 else None
    if m2 is not None:
        m2[0, 0] = 1.0
    logp = torch.log_softmax(seeded("nll.l", (B, T, V)), 2).contiguous()
    sums, dlogp, sd = nanf(2), nanf(B, T, V), torch.tensor([0.75], device="cuda")
    call("xg_nll_fwd", _S(), ptr(logp), ptr(tgt), ptr(mask), ptr(m2), B, T, V, roll, ptr(sums))
    call("xg_nll_bwd", _S(), ptr(tgt), ptr(mask), ptr(m2), B, T, V, roll, ptr(sums), 2.0, ptr(sd), ptr(dlogp))
    torch.cuda.synchronize()
    m = mask.double().cpu().numpy() * (1.0 if m2 is None else m2.double().cpu().numpy())
    t = tgt.cpu().numpy()
    t = np.concatenate([t[:, 1:], t[:, :1]], 1) if roll else t
    want = np.zeros((B, T, V))
    np.put_along_axis(want, t[:, :, None], (-2.0 * 0.75 * m / m.sum())[:, :, None], 2)
    lp = logp.double().cpu().numpy()
    assert abs(float(sums[1]) - m.sum()) == 0 and abs(float(sums[0]) + (np.take_along_axis(lp, t[:, :, None], 2)[:, :, 0] * m).sum()) < 1e-4
    got = dlogp.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    assert (got[1] == 0).all()


@pytest.mark.parametrize("with_n", [False, True])
def test_criteria_reward_backward_overwrites_dslp(with_n):
    """xg_reward_bwd: every element of a NaN-filled dslp = -scale_dev * reward[b] * mask / sum(mask) (rs_t = 0: one reward per
    video; mask[:, 0] = 1, mask[:, t] = seq[:, t-1] > 0, columns >= n_dev masked), float64 formula, 4 ulp as above."""
    m, L = 6, 9
    seq = torch.from_numpy(pg.randint("rw.s", (m, L), 4, 1, 50)).cuda()
    seq[1, 0:] = 0
    seq[2, 3:] = 0
    seq[4, 6:] = 0
    reward = seeded("rw.r", (m,))
    n = 7
    nd = torch.tensor([n], dtype=torch.int32, device="cuda") if with_n else None
    slp = -seeded("rw.l", (m, L), 0.1, 3.0)
    sums, dslp, sd = nanf(2), nanf(m, L), torch.tensor([1.5], device="cuda")
    call("xg_reward_fwd", _S(), ptr(slp), L, ptr(seq), L, ptr(reward), 1, 0, ptr(nd), m, L, ptr(sums))
    call("xg_reward_bwd", _S(), ptr(seq), L, ptr(reward), 1, 0, ptr(nd), m, L, ptr(sums), ptr(sd), ptr(dslp), L)
    torch.cuda.synchronize()
    s = seq.cpu().numpy()
    mask = np.concatenate([np.ones((m, 1)), (s[:, :-1] > 0).astype(np.float64)], 1)
    if with_n:
        mask[:, n:] = 0
    rw = reward.double().cpu().numpy()[:, None]
    want = -1.5 * rw * mask / mask.sum()
    assert float(sums[1]) == mask.sum()
    assert abs(float(sums[0]) + (slp.double().cpu().numpy() * rw * mask).sum()) < 1e-4
    got = dslp.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    assert (got[mask == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------- (e)
def test_pool_poisoned_between_training_iterations():
    """(i) The loop of test_overlapped_update_equals_plain_update with ClipAdam(overlap=True, fused_zero=True); every workspace of
    the pool poisoned between iterations: the parameters of the unpoisoned loop, under that test's own bounds."""
    from controllable_xgating_amd.train import ClipAdam
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    out = []
    for poisoned in (False, True):
        model = make_model(d)
        opt = ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=True, fused_zero=True)
        for _ in range(3):
            opt.zero_grad()
            loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
            opt.arm()
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            assert wss.pool_sync_words_zero(model)
            if poisoned:
                assert wss.poison_pool(model) >= 1
        torch.cuda.synchronize()
        out.append(({n: q.detach().clone() for n, q in model.named_parameters()}, float(loss.detach())))
    (p0, l0), (p1, l1) = out
    assert abs(l0 - l1) < 1e-5, (l0, l1)
    for n in p0:
        assert bool(torch.isfinite(p1[n]).all()), n
        if n in ZERO_GRAD_PARAMS:
            continue
        assert float((p0[n] - p1[n]).abs().max()) < 5e-6, n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pool_poisoned_between_xe_scst_and_eval_stages(precision):
    """(ii) XE iteration -> sample_pair + reward backward -> eval forward + greedy sample -> XE iteration, as a training script
    interleaves them, the pool poisoned between the stages: every stage's results equal those of the unpoisoned sequence."""
    from controllable_xgating_amd import RewardCriterion
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    u = torch.from_numpy(pg.uniform("uni_pool", (d.L + 1, d.B), 5)).cuda()
    args = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"])
    runs = []
    for poisoned in (False, True):
        model = make_model(d, precision=precision)
        rec = []

        def between():
            torch.cuda.synchronize()
            assert wss.pool_sync_words_zero(model)
            if poisoned:
                assert wss.poison_pool(model) >= 1

        def xe():
            model.flat_grads().zero_()
            loss = model.xe_loss(*args, x["seq"], x["seq_mask"], x["cap_classes"], x["class_mask"], WEIGHT_CLASS)
            loss.backward()
            rec.append(dict(loss=loss.detach().reshape(1).clone(), g=model.flat_grads().detach().clone()))
        xe()
        between()
        model.flat_grads().zero_()
        gen, slp, greedy, n = model.sample_pair(*args, {"uniforms": u})
        loss = RewardCriterion()(slp, gen, torch.full_like(slp, 0.25))
        loss.backward()
        rec.append(dict(loss=loss.detach().reshape(1).clone(), g=model.flat_grads().detach().clone(), gen=gen.clone(), greedy=greedy.clone(),
                        n=n.clone(), slp=slp.detach().clone()))
        between()
        model.eval()
        with torch.no_grad():
            logp, cat = model(*args, x["seq"], x["seq_mask"])
            seq, lp = model.sample(*args, {"sample_max": 1, "async": True})[:2]
        rec.append(dict(logp=logp.clone(), cat_logp=cat.clone(), seq=seq.clone(), seq_logp=lp.clone()))
        model.train()
        between()
        xe()
        between()
        runs.append(rec)
    for i, (a, b) in enumerate(zip(*runs)):
        same_as(a, b, "%s stage %d" % (precision, i))


def test_pool_poisoned_between_graph_replays():
    """(iii) train.GraphedXEStep: the pool poisoned between replays; losses and parameters of unpoisoned replays under the bounds
    of test_graphed_xe_step_equals_the_eager_loop.  A clear done at capture time instead of being captured shows here."""
    from controllable_xgating_amd import train as tr
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    outs = []
    for poisoned in (False, True):
        model = make_model(d, P=Pn, train=True)
        opt = tr.ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=True, fused_zero=True, device_state=True)
        step = tr.GraphedXEStep(model, opt, x, weight_class=WEIGHT_CLASS)
        losses = []
        for _ in range(4):
            torch.cuda.synchronize()
            if poisoned:
                assert wss.poison_pool(model) >= 1
            losses.append(float(step().item()))
            torch.cuda.synchronize()
            assert wss.pool_sync_words_zero(model)
        outs.append((losses, model.flat_parameters().detach().cpu().numpy().copy()))
    (l0, p0), (l1, p1) = outs
    assert np.isfinite(l1).all() and np.isfinite(p1).all(), l1
    np.testing.assert_allclose(l1, l0, atol=2e-5)
    disp = np.abs(p1 - p0)
    assert disp.max() <= 4.1 * 4e-4 and (disp > 4e-5).mean() <= 0.02, (float(disp.max()), float((disp > 4e-5).mean()))


# ---------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("cfg", ["A", "E"])
def test_negative_control_poison_between_forward_and_backward_breaks_the_gradients(cfg):
    """The tests above can fail: poison() BETWEEN xg_forward_xe and xg_backward_xe (a breach of the contract; data words and valid
    integers only, the synchronisation words untouched) reaches the saved activations and the gradients come out non-finite."""
    r = Rig(**CONFIGS[cfg])
    d = r.dims()
    B, T = d.B, d.T
    wp, wn = r.ws("ws1", d)
    logp, cat = nanf(B, T, d.V), nanf(B, T, d.C)
    bn, _ = r.bn()
    run, b = r.run(1), r.batch()
    call("xg_forward_xe", _S(), C.byref(d), C.byref(r.ps), C.byref(bn), C.byref(b), C.byref(run), wp, wn, ptr(logp), ptr(cat))
    r.poison_all()
    r.g.zero_()
    dl, dc = seeded("dlogp", (B, T, d.V)) / (B * T), seeded("dcat", (B, T, d.C)) / (B * T)
    call("xg_backward_xe", _S(), C.byref(d), C.byref(r.ps), C.byref(r.gs), C.byref(b), C.byref(run), wp, wn, ptr(dl), ptr(dc))
    assert r.sync_zero()
    assert bool(torch.isfinite(logp).all())
    assert not bool(torch.isfinite(r.g).all())
