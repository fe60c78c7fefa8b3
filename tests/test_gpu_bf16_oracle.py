"""precision="bf16" (XgRun.gemm_mode 1) against the float64 oracle that rounds where the kernels round (tests/bf16_oracle.py).

Every other whole-model check of this mode compares with the fp32 oracle, so its bounds have to absorb the bf16 rounding itself
(loss 1e-2, gradient norms 5 %, cosine 0.997).  Here the reference rounds the same operands at the same places, what is left is
accumulation order and the operands that round the other way, and the bounds are FLOOR_MARGIN times that measured floor: the fp32
path's own 1e-4 on the loss, 2e-3 .. 6e-3 of the scale on every gradient (measured on MI355X: at most 1.9 x the floor).

Stage 3: one decoder step (xg_step_fwd + xg_step_bwd) -- packed bf16 tiles, the LDS-staged kernel without them, the scalar-load
form on unaligned extents, and extents the skinny launcher does not take at all.
Stage 4: teacher-forced forward + backward with both criteria at tests/bf16_oracle.py: XE_DIMS -- dense, ragged, dropout 0.5 on
the oracle's hash masks, and a workspace without the mirror region (every consumer converts on the fly).
Every figure is printed before it is asserted (pytest -s shows them; docs/EXPERIMENTS.md records a run)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bf16_oracle as bo
from tests.util import WEIGHT_CLASS, ZERO_GRAD_PARAMS, grad_misses, make_model, model_grads, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


# ---------------------------------------------------------------------------------------------------- stage 3
def _hip_step(tag, packed):
    """xg_step_fwd (save = 1) + xg_step_bwd in gemm_mode 1 on step_inputs(tag); packed=False: XgRun.packed = NULL (the LDS-staged
    sk_kernel<., 1>).  -> the same dict as bo.step_oracle."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _grads_struct, _stream, _ws_ptr
    d, Pn, x = bo.step_inputs(tag)
    B, K, R, A = d.B, d.K, d.R, d.A
    model = make_model(d, P=Pn, train=True, precision="bf16")
    model.flat_grads().zero_()
    dd, ps, run = model._dims(B, K, 1), model._params_struct(), model._run(True)
    assert run.gemm_mode == 1
    if packed:
        assert run.packed and run.packed_dtype == 1, "this case is about the packed bf16 tiles"
    else:
        run.packed = None
    g, gs = _grads_struct(model, "cuda")
    assert g is None
    L = nv.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    Vd, posd, vpd, tokd, mkd = dev(x["V"]), dev(x["pos"]), dev(x["vproj"]), dev(x["tok"]), dev(x["mk"])
    state = dev(x["st"])
    wp, wnb = _ws_ptr(model._pool.shared(dd, Vd.device))
    alpha = torch.zeros(B, K, device="cuda")
    nv.check(L.xg_step_fwd(_stream(), C.byref(dd), C.byref(ps), nv.ptr(tokd), nv.ptr(mkd), nv.ptr(Vd), nv.ptr(vpd), nv.ptr(posd),
                           C.byref(run), 3, wp, wnb, nv.ptr(state), None, nv.ptr(alpha)), "xg_step_fwd")
    new = state.clone()
    dst_new = dev(x["w"])
    dst = torch.full((4, B, R), 7.0, device="cuda")                        # overwritten
    dV, dvp, dpos = torch.zeros(B, K, R, device="cuda"), torch.zeros(B, K, A, device="cuda"), torch.zeros(B, R, device="cuda")
    nv.check(L.xg_step_bwd(_stream(), C.byref(dd), C.byref(ps), C.byref(gs), nv.ptr(tokd), nv.ptr(mkd), nv.ptr(Vd), nv.ptr(vpd),
                           nv.ptr(posd), C.byref(run), 3, wp, wnb, nv.ptr(state), nv.ptr(dst_new), nv.ptr(dst), nv.ptr(dV),
                           nv.ptr(dvp), nv.ptr(dpos)), "xg_step_bwd")
    torch.cuda.synchronize()
    f = lambda t: t.detach().cpu().double().numpy()                        # noqa: E731
    out = dict(h1=f(new[0]), c1=f(new[1]), h2=f(new[2]), c2=f(new[3]), alpha=f(alpha), dstate=f(dst), dV=f(dV), dvproj=f(dvp), dpos=f(dpos))
    grads = model_grads(model)
    out["grads"] = {k: grads[k].astype(np.float64) for k in bo.step_oracle(tag)["grads"]}
    return out


def _step_figures(got, ref):
    """[(quantity, max error, largest reference entry, bound)] of one step"""
    rows = []
    for k, key in (("h1", "state"), ("c1", "state"), ("h2", "state"), ("c2", "state"), ("alpha", "alpha"), ("dstate", "dstate"),
                   ("dV", "dV"), ("dvproj", "dvproj"), ("dpos", "dpos")):
        scale = float(np.abs(ref[k]).max())
        rows.append((k, float(np.abs(got[k] - ref[k]).max()), scale, bo.FP32_GRAD_ATOL + bo.step_rtol(key) * scale))
    for name, r in ref["grads"].items():
        scale = float(np.abs(r).max())
        rows.append((name, float(np.abs(got["grads"][name] - r).max()), scale, bo.FP32_GRAD_ATOL + bo.step_rtol("grads") * scale))
    return rows


STEP_RUNS = [("mid", True), ("mid", False), ("r8_unaligned", False), ("odd", False)]
_STEP = {}


def _step(tag, packed):
    if (tag, packed) not in _STEP:
        _STEP[(tag, packed)] = _hip_step(tag, packed)
    return _STEP[(tag, packed)]


@pytest.mark.parametrize("tag,packed", STEP_RUNS)
def test_one_decoder_step_bf16_vs_rounding_oracle(tag, packed):
    """xg_step_fwd + xg_step_bwd in gemm_mode 1 with one or two held rows: new state, alpha, dstate, dV, dvproj, dpos and every
    lstmcore / embed gradient against core_step in float64 under hip_bf16_policy(d, "step") -- every forward product of the step
    rounds both operands (R % 8 == 0), the backward is exact fp32 on what the forward saved (xg_step_bwd: gemm_mode 0).
    mid + packed: skf_kernel<., 1> on bf16 tiles; mid without: sk_kernel<true, 1>; r8_unaligned: sk_kernel<false, 1> (E, A not
    multiples of 4); odd: R % 8 != 0, plain GEMMs far below the 256 / 64 / 256 rule -- nothing rounds, and the policy says so."""
    d, _, _ = bo.step_inputs(tag)
    sites = bo.rounding_sites(d, "step")
    assert len(sites) == (8 if d.R % 8 == 0 else 0) and all(k == "fwd" for _, k in sites), sites
    ref, got = bo.step_oracle(tag), _step(tag, packed)
    rows = _step_figures(got, ref)
    for name, err, scale, lim in rows:
        print("step %s packed=%d %-32s err %.3e scale %.3e bound %.3e" % (tag, packed, name, err, scale, lim))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad
    if sites:
        # the roundings are what this reference adds: the plain float64 oracle is further from the kernel than the bound on the
        # new state (so a step that rounded nothing, or only one operand, would not pass above)
        plain = bo.step_oracle(tag, policy=None)
        far = max(float(np.abs(got[k] - plain[k]).max() / np.abs(plain[k]).max()) for k in ("h1", "c1", "h2", "c2"))
        near = max(float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in ("h1", "c1", "h2", "c2"))
        print("step %s packed=%d state vs plain oracle %.3e, vs rounding oracle %.3e" % (tag, packed, far, near))
        assert far > 10 * near, (far, near)


def test_one_decoder_step_packed_and_generic_tile_paths_agree():
    """The same step through the packed bf16 tiles and through the LDS-staged kernel: the same rounded operands, another
    accumulation order -- every output within the step's bound of the other path."""
    a, b = _step("mid", True), _step("mid", False)
    rows = _step_figures(b, dict(a, grads=a["grads"]))
    for name, err, scale, lim in rows:
        print("step packed vs generic %-32s err %.3e scale %.3e bound %.3e" % (name, err, scale, lim))
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- stage 4
_XE = {}


def _hip_xe(ragged, p, mirrors):
    """model(...) + both criteria + backward with precision="bf16" on the inputs of bo.xe_oracle(ragged, p, mirrors); mirrors=False:
    the pool sizes its workspaces by xg_workspace_bytes_mode(d, 0) -- no mirror region, every consumer converts on the fly."""
    key = (ragged, p, mirrors)
    if key in _XE:
        return _XE[key]
    from controllable_xgating_amd import ClassiferCriterion, LanguageModelCriterion
    from controllable_xgating_amd import _native as nv
    ref = bo.xe_oracle(ragged, p, mirrors)
    d = ref["d"]
    model = make_model(d, P=ref["Pn"], p_drop=p, precision="bf16")
    model.dropout_seed = bo.XE_SEED
    if not mirrors:
        model._pool.gemm_mode = 0
    x = to_dev(ref["xn"])
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    l_xe = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    l_cls = ClassiferCriterion()(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    (bo.XE_LOSS_GAIN * (l_xe + WEIGHT_CLASS * l_cls)).backward()
    torch.cuda.synchronize()
    dd = model._dims(d.B, d.K, d.L + 1)
    n0, n1 = (nv.lib().xg_workspace_bytes_mode(C.byref(dd), m) for m in (0, 1))
    sizes = {ws.numel() - 256 for lst in model._pool.free.values() for ws in lst}
    assert n0 < n1 and sizes == {n1 if mirrors else n0}, (sizes, n0, n1)
    _XE[key] = dict(logp=logp.detach().cpu().double().numpy(), cat=cat.detach().cpu().double().numpy(), l_xe=l_xe.item(), l_cls=l_cls.item(),
                    grads={k: v.astype(np.float64) for k, v in model_grads(model).items()})
    return _XE[key]


def _xe_check(got, ref, tag, exempt=None, skip=()):
    """Print and collect what misses the stage-4 bounds: losses, log-probs, every gradient (grad_misses with the parameter's own
    rtol, the ReLU-flip exemptions of the reference)."""
    bad = []
    for k in ("l_xe", "l_cls"):
        print("%s %-8s hip %.7f ref %.7f diff %.2e bound %.1e" % (tag, k, got[k], ref[k], abs(got[k] - ref[k]), bo.XE_LOSS_TOL))
        if not abs(got[k] - ref[k]) < bo.XE_LOSS_TOL:
            bad.append((k, got[k], ref[k]))
    dl, dc = got["logp"] - ref["logp"], got["cat"] - ref["cat"]
    figs = (("logp max", float(np.abs(dl).max()), bo.XE_LOGP_TOL), ("logp rms", float(np.sqrt((dl ** 2).mean())), bo.XE_LOGP_RMS_TOL),
            ("cat max", float(np.abs(dc).max()), bo.XE_CAT_TOL))
    for name, v, lim in figs:
        print("%s %-8s %.3e bound %.1e" % (tag, name, v, lim))
        if not v <= lim:
            bad.append((name, v, lim))
    rep = {}
    for name in ref["grads"]:
        if name in ZERO_GRAD_PARAMS or name in skip:
            continue
        bad += grad_misses({name: got["grads"][name]}, ref["grads"], rtol=bo.xe_grad_rtol(name), atol=bo.FP32_GRAD_ATOL,
                           cos_min=bo.XE_COS_MIN, exempt=exempt, report=rep, elem_share=bo.XE_ELEM_SHARE)
    for name, (rel, cos, elem, nex) in rep.items():
        fl = bo.XE_GRAD_FLOOR[name]
        print("%s grad %-52s err/scale %.2e (floor %.1e, x%.1f; bound %.1e)  1-cos %.1e  exempt %d"
              % (tag, name, rel, fl, rel / max(fl, 1e-12), bo.xe_grad_rtol(name), 1 - cos, nex))
    return bad


def test_xe_dims_put_products_on_both_sides_of_the_rule():
    """XE_DIMS: which product runs on the bf16 kernels and which stays fp32 follows from the 256 / 64 / 256 rule -- asserted, so
    that a later change of the dims cannot silently move everything to one side."""
    d = bo.xe_dims()
    tab = bo.xe_expected_sides(d)
    assert d.B * d.K >= 256 and (d.L + 1) // 2 * d.B >= 256
    assert tab[("logit", "fwd")][3] and tab[(bo.ENC + "visual_emb_rgb.0", "fwd")][3] and not tab[(bo.ENC + "visual_emb_opfl.0", "fwd")][3]
    assert tab[("logit", "db")][3] and not bo.policy_table(d, "xe", mirrors=False)[("logit", "db")][3]


@pytest.mark.parametrize("ragged,p,mirrors", bo.XE_CASES, ids=["dense", "ragged", "dropout", "ragged_no_mirror_workspace"])
def test_xe_bf16_vs_rounding_oracle(ragged, p, mirrors):
    """Teacher-forced forward + backward, both criteria, precision="bf16": losses, log-probs and every parameter gradient against
    forward_xe + lm_criterion + cls_criterion in float64 under hip_bf16_policy(d, "xe")."""
    ref, got = bo.xe_oracle(ragged, p, mirrors), _hip_xe(ragged, p, mirrors)
    print("flip candidates", ref["counts"])
    bad = _xe_check(got, ref, "xe ragged=%d p=%.1f mirrors=%d" % (ragged, p, mirrors), ref["exempt"])
    assert not bad, bad


def test_xe_bf16_mirrorless_workspace_agrees_with_the_mirrored_run():
    """The same call on a workspace with and without the mirror region: the same rounded operands (a mirror is the rounding of the
    fp32 value), other kernels; the bias gradients that ride in the weight-gradient products sum the mirror in one run and the
    fp32 values in the other: those biases (the policy tables of the two workspaces name them) are held by each run's own oracle
    above, every other output is within the stage-4 bounds of the other run."""
    d = bo.xe_dims()
    with_m, without = bo.policy_table(d, "xe", mirrors=True), bo.policy_table(d, "xe", mirrors=False)
    differ = {k for k in with_m if with_m[k][3] != without[k][3]}
    assert differ and all(kind in ("db", "grad") for _, kind in differ), differ
    a, b = _hip_xe(True, 0.0, True), _hip_xe(True, 0.0, False)
    # site -> its bias: "<prefix>.bias", or the LSTMCell's bias_ih / bias_hh beside weight_ih / weight_hh
    skip = {site.replace("weight_", "bias_") if "weight_" in site else site + ".bias" for site, kind in differ if kind == "db"}
    assert skip <= set(a["grads"]), skip
    print("bias gradients summed from the mirror in one run only:", sorted(skip))
    assert "logit.bias" in skip and "classifer.0.bias" not in skip and "lstmcore.v2a.bias" not in skip
    bad = _xe_check(b, a, "xe no-mirror vs mirror", skip=skip)
    assert not bad, bad
