"""TEST INFRASTRUCTURE ONLY -- the float64 oracle that rounds where the HIP path of precision="bf16" (XgRun.gemm_mode 1) rounds.

oracle/xgate_oracle.py routes every product through ``_mm(x, W, site, policy)``; ``hip_bf16_policy`` below is the policy that says,
site by site and kind by kind, whether the HIP path rounds the operands of that product to bf16 (DESIGN.md 4.2 has the same table
with the source lines).  Against this reference a bf16 run differs only by accumulation order -- and by the operands that sit within
fp32 round-off of a bf16 rounding boundary and round the other way (the bf16 analogue of a flipped ReLU derivative).

The rules, read from the code (csrc/xg_gemm.hip: xgk_gemm_cs / xgk_gemm_x, csrc/xg_step.hip: xgk_skinny, csrc/xg_model.hip):
  rule    a product issued as a GEMM (lin16 / nn16 / tn16 / xgk_linear / gemm_nn / gemm_tn_cs) runs on the bf16 matrix cores, BOTH
          operands rounded, when M >= 256 and N >= 64 and K >= 256 as the kernel sees them (forward rows x out x in; data gradient
          rows x in x out; weight gradient out x in x rows); otherwise it is exact fp32.  A bf16 mirror holds the rounding of the fp32
          value, so reading the mirror and converting on the fly are the same numbers.
  step    a per-step product (xgk_skinny) rounds both operands whatever its shape -- when the skinny launcher takes it: forward
          R % 8 == 0 (init_hidden: R % 4 == 0), data gradient R % 4 == 0.  Otherwise the same product goes out as a GEMM: rule.
  db      a bias gradient that rides in a weight-gradient product as column sums is summed over the bf16 MIRROR of dY when that
          product runs on the bf16 kernels and reads the mirror (16-byte loadable: the out extent a multiple of 8); a workspace
          without a mirror region sums the fp32 values.  Bias gradients with a pass of their own (xgk_colsum*, gemm_tn_cs without
          mirrors) sum fp32 values: embeddings, img_embed_*, POS gate, classifier, and v2a.bias on purpose (xg_model.hip:1092).
  never   the attention's a2w scoring runs inside the attention kernels in fp32; xg_step_bwd sets gemm_mode 0 for the whole
          single-step backward (xg_model.hip:1473).
  halves  the teacher-forced vocabulary product is issued as two GEMMs (steps [0, T/2) under the remaining steps, then the rest)
          when the side streams are on and T >= 4: each half meets the rule with its own rows (xg_model.hip:841-855, 873-879).
The rounding itself is round-to-nearest-even everywhere (xg_step.hip:88 bf16_rne and :96 v_cvt_pk_bf16_f32, xg_gemm_bf16.hip:594-611,
xg_pack.hip:103,118): oracle ``rb``.

THE FLOOR.  The emulated oracle run in float32 (operands computed in fp32, then rounded like the kernels) against the same in float64
differs where an operand rounds the other way.  That difference is what any fp32-accumulating implementation has against the
float64 emulation, so the bounds below are FLOOR_MARGIN times it, never tighter than the fp32 path's own bounds and never looser
than a tenth of the bf16 bound beside which they stand (tests/test_gpu_fullsize.py: 5 % of the scale, cosine 0.997; loss 1e-2).
Measured floors (CPU; tests/test_bf16_oracle_cpu.py recomputes them, docs/EXPERIMENTS.md has the account):
  stage 3, one decoder step (STEP_CASES): max |f32 - f64| / max |f64| 1e-7 .. 1.4e-6, cosine 1 to fp32 round-off -- fp32 class: a
           step has too few computed operands for one to sit on a rounding boundary.  Bounds: the fp32 path's own 2e-3 / 2e-6.
  stage 4, teacher-forced XE at XE_DIMS (XE_CASES: dense, ragged, dropout 0.5, mirror-less workspace): loss 1.3e-5, log-probs
           9.4e-4 (rms 9.3e-5), category log-probs 7.0e-4, gradients 2e-5 .. 3.6e-3 of the scale (XE_GRAD_FLOOR, worst: the two
           embedding matrices in front of BatchNorm), 1 - cosine <= 7.1e-6.  One float64 run takes 2 s.
  the rollout case row_pass_bf16 of tests/test_gpu_rollout_oracle.py (`mid`: only the step products round): loss 1e-7, gathered
           log-probs 1.1e-5, the two emulations draw the same tokens at both temperatures.  Bounds: the fp32 path's own.
What the stage-4 inputs owe to the floor condition (every gradient <= 5e-3, loss <= 1e-3): XE_RELU_BIAS_SHIFT, XE_FRAME_RAMP,
XE_LOSS_GAIN and dropout on the dense captions -- each explained where it is defined.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG, WEIGHT_CLASS, ZERO_GRAD_PARAMS, flip_exemptions, run_oracle  # noqa: F401 (CFG: re-exported)

ENC = xo.ENC
KINDS = ("fwd", "dx", "dw", "db")


def rule(M, N, K):
    """csrc/xg_gemm.hip: xgk_gemm_cs / xgk_gemm_x -- the products large enough for the bf16 tile kernels."""
    return M >= 256 and N >= 64 and K >= 256


def policy_table(d, entry, T=None, mirrors=True, overlap=True):
    """{(site, kind): (M, N, K, rounds, why)} of the HIP path in gemm_mode 1 for dims `d`.  entry: "xe" (xg_forward_xe +
    xg_backward_xe with both criteria), "rollout" (xg_rollout with saved activations + xg_rollout_bwd: every product of the step is
    a step product, the vocabulary product one GEMM per step, the backward that of "xe" over the T - 1 steps the rollout runs, no
    classifier), "step" (xg_step_fwd + xg_step_bwd: the rollout form of the step, exact-fp32 backward).
    M, N, K: what the kernel sees (for a product issued in two halves: the smaller half's rows)."""
    B, K, R, A, E, V, C, H = d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H
    T = d.L + 1 if T is None else T
    roll = entry == "rollout"
    if roll:
        T -= 1                                                                                 # xg_model.hip:1866
    N, TB = B * K, T * B
    step = entry == "step"
    tab = {}

    def put(site, kind, M_, N_, K_, rounds, why):
        tab[(site, kind)] = (M_, N_, K_, bool(rounds), why)

    def gemm(site, rows, out, inn, db=None, kinds=("fwd", "dx", "dw")):
        """a product issued as GEMMs in all directions; db: None (own fp32 pass) or the (out, in, rows) of the product it rides in"""
        for kind, (M_, N_, K_) in (("fwd", (rows, out, inn)), ("dx", (rows, inn, out)), ("dw", (out, inn, rows))):
            if kind in kinds:
                put(site, kind, M_, N_, K_, rule(M_, N_, K_), "rule")
        ride(site, db)

    def ride(site, db):
        if db is None:
            put(site, "db", 0, 0, 0, False, "own fp32 pass")
        else:
            M_, N_, K_ = db
            put(site, "db", M_, N_, K_, mirrors and rule(M_, N_, K_) and M_ % 8 == 0, "column sums of the dY mirror" if mirrors else "no mirror: fp32 sums")

    def stepp(site, out, inn, dw_rows, db, fwd_mod=8):
        """a per-step product: forward and data gradient through xgk_skinny, weight gradient batched over dw_rows"""
        sk_f, sk_b = R % fwd_mod == 0, R % 4 == 0
        put(site, "fwd", B, out, inn, sk_f or rule(B, out, inn), "step" if sk_f else "rule")
        put(site, "dx", B, inn, out, sk_b or rule(B, inn, out), "step" if sk_b else "rule")
        put(site, "dw", out, inn, dw_rows, rule(out, inn, dw_rows), "rule")
        ride(site, db)

    if step:
        # xg_step_fwd: every product of the step through xgk_skinny (R % 8 == 0) or plain GEMMs; xg_step_bwd: gemm_mode 0
        for site, out, inn in (("lstmcore.gate.gate.0", R, E), ("lstmcore.h2a", A, R),
                               ("lstmcore.lstm_1.i2h", 4 * R, E), ("lstmcore.lstm_1.a2h", 4 * R, R), ("lstmcore.lstm_1.h2h", 4 * R, R),
                               ("lstmcore.lstm_2.i2h", 4 * R, R), ("lstmcore.lstm_2.a2h", 4 * R, R), ("lstmcore.lstm_2.h2h", 4 * R, R)):
            sk = R % 8 == 0
            put(site, "fwd", B, out, inn, sk or rule(B, out, inn), "step" if sk else "rule")
            for kind in ("dx", "dw", "db"):
                put(site, kind, 0, 0, 0, False, "xg_step_bwd: gemm_mode 0")
        for kind in KINDS:
            put("lstmcore.a2w", kind, 0, 0, 0, False, "attention kernels: fp32")
        put("logit.out", "val", 0, 0, 0, False, "-")
        put("logit.out", "grad", 0, 0, 0, False, "-")
        return tab
    # ---- encoder
    for mod, F in (("rgb", d.F1), ("opfl", d.F2)):
        gemm(ENC + f"visual_emb_{mod}.0", N, R, F, kinds=("fwd", "dw"))                        # xg_model.hip:351, 510
        put(ENC + f"visual_emb_{mod}.0", "dx", N, F, R, False, "no gradient wrt the features")
        whh_dw = (4 * R, R, N)                                                                 # :499 carries bias_ih and bias_hh
        gemm(ENC + f"lstmcell_{mod}.weight_ih", N, 4 * R, R, db=whh_dw)                        # :371, 503, 500
        stepp(ENC + f"lstmcell_{mod}.weight_hh", 4 * R, R, N, db=whh_dw)                       # :394 / 398, 482, 499
        gemm(ENC + f"gate_{mod}.gate.0", N, R, R, db=(R, R, N))                                # :408-409, 441, 440
    gemm(ENC + "fusion.late_fusion.0", N, R, 2 * R, db=(R, 2 * R, N))                          # :414, 432, 431
    # ---- decoder
    for n in ("img_embed_h_1", "img_embed_c_1", "img_embed_h_2", "img_embed_c_2"):
        sk = R % 4 == 0
        put(n, "fwd", B, R, R, sk or rule(B, R, R), "step" if sk else "rule")                  # :523-532
        put(n, "dx", B, R, R, False, "vbar is detached")
        put(n, "dw", R, R, B, rule(R, R, B), "rule")                                           # :1078
        ride(n, None)
    gemm("lstmcore.v2a", N, A, R, db=None)                                                     # :540, 1070, 1096 (bias: :1097)
    stepp("lstmcore.h2a", A, R, TB, db=(A, R, TB))                                             # :655-660, 931 / 1037, 990-991
    for kind in KINDS:
        put("lstmcore.a2w", kind, 0, 0, 0, False, "attention kernels: fp32")
    l1_dw = (4 * R, R, TB)                                                                     # :1001 carries the three lstm_1 biases
    gemm("lstmcore.gate.gate.0", TB, R, E, db=None)                                            # :819, 1088, 1087
    gemm("lstmcore.lstm_1.i2h", TB, 4 * R, E, db=l1_dw)                                        # :822, 1006, 1002
    gemm("lstmcore.lstm_1.a2h", TB, 4 * R, R, db=l1_dw)                                        # :824, 1005, 1003
    if roll:    # the token side is not hoisted: three more products of the step (:648-654, 719-727 / 768-777, 792-801)
        for site, out, inn in (("lstmcore.gate.gate.0", R, E), ("lstmcore.lstm_1.i2h", 4 * R, E), ("lstmcore.lstm_1.a2h", 4 * R, R)):
            sk = R % 8 == 0
            put(site, "fwd", B, out, inn, sk or rule(B, out, inn), "step" if sk else "rule")
    stepp("lstmcore.lstm_1.h2h", 4 * R, R, TB, db=l1_dw)                                       # :702, 952, 1001
    for n in ("i2h", "a2h", "h2h"):
        stepp("lstmcore.lstm_2." + n, 4 * R, R, TB, db=(4 * R, R, TB))                         # :738-740, 929 / 1024-1025, 987-989
    # ---- heads
    th = T // 2 if (overlap and T >= 4) else 0
    halves = [r for r in (th * B, (T - th) * B) if r > 0]
    if roll:
        put("logit", "fwd", B, V, R, rule(B, V, R), "rule, per step")                          # :1729
        sides = {rule(r, R, V) for r in halves}                                                # :1133 (no classifier: two halves)
        assert len(sides) == 1, ("the two halves of the vocabulary data gradient fall on different sides of the rule", halves)
        put("logit", "dx", min(halves), R, V, sides.pop(), "rule, per half")                   # :1145, 1152
    else:
        sides = {rule(r, V, R) for r in halves}
        assert len(sides) == 1, ("the two halves of the vocabulary product fall on different sides of the rule", halves)
        put("logit", "fwd", min(halves), V, R, sides.pop(), "rule, per half")                  # :854, 878
        put("logit", "dx", TB, R, V, rule(TB, R, V), "rule")                                   # :1145 (both criteria: one product)
    put("logit", "dw", V, R, TB, rule(V, R, TB), "rule")                                       # :1157
    ride("logit", (V, R, TB))
    # dlogits: the fused loss path writes its bf16 copy itself (xg_heads.hip:253), every other producer is followed by cvt16
    # (:1139) -- the same numbers, and nothing but the two vocabulary products and their column sums reads them
    put("logit.out", "val", TB, V, 0, False, "-")
    put("logit.out", "grad", TB, V, 0, tab[("logit", "db")][3], "the dlogits mirror (read by dx, dw and the column sums)")
    if not roll:
        gemm("classifer.0", TB, H, R, db=None)                                                 # :867, 1170, 1169
        gemm("classifer.3", TB, C, H, db=None)                                                 # :869, 1167, 1166
    return tab


def truncate_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (what a conversion without the rounding increment computes): a WRONG rule"""
    u = x.detach().to(torch.float32).contiguous().view(torch.int32) & -65536
    return u.view(torch.float32).to(x.dtype)


def hip_bf16_policy(d, entry="xe", T=None, mirrors=True, overlap=True, omit=(), truncate=()):
    """The policy of the HIP path (policy_table).  omit: (site, kind) pairs whose rounding is left out; truncate: pairs that round
    by truncation -- the mutated policies of the discrimination test.  A site the table does not know is an error: a new product
    has to be entered."""
    tab = policy_table(d, entry, T, mirrors, overlap)
    omit, truncate = set(omit), set(truncate)
    for key in omit | truncate:
        assert tab[key][3], (key, "does not round: a mutation here changes nothing")

    def policy(site, kind, M, N, K):
        if (site, kind) in truncate:
            return truncate_bf16
        return tab[(site, kind)][3] and (site, kind) not in omit
    return policy


def rounding_sites(d, entry="xe", **kw):
    """The (site, kind) pairs that round, sorted."""
    return sorted(k for k, v in policy_table(d, entry, **kw).items() if v[3])


# ---------------------------------------------------------------------------------------------------- bounds
FLOOR_MARGIN = 4.0
# the fp32 path's own bounds (tests/util.py: grad_misses; test_xe_forward_backward_vs_oracle) -- never tighter than these
FP32_GRAD_RTOL, FP32_GRAD_ATOL, FP32_LOSS_TOL, FP32_LOGP_TOL, FP32_CAT_TOL, FP32_COS = 2e-3, 2e-6, 1e-4, 3e-4, 1e-4, 1 - 1e-5
# a tenth of today's bf16 bounds (5 % of the scale, cosine 0.997, loss 1e-2, log-probs 1e-2) -- never looser than these
CAP_GRAD_RTOL, CAP_LOSS_TOL, CAP_LOGP_TOL, CAP_COS = 5e-3, 1e-3, 1e-3, 1 - 3e-4


def bound(floor, lo, cap):
    """FLOOR_MARGIN x floor, inside [lo, cap]"""
    return float(min(max(FLOOR_MARGIN * floor, lo), cap))


# Measured floors (tests/test_bf16_oracle_cpu.py: test_floor_* recompute them and fail if one is above its entry here).
# stage 3, worst of the four cases of STEP_CASES; relative to the largest entry of the float64 reference
STEP_FLOOR = dict(state=1.7e-7, alpha=1.7e-7, dstate=1.6e-7, dV=3.1e-7, dvproj=7.0e-7, dpos=2.3e-7, grads=1.4e-6)
# stage 4, worst of dense / ragged / dropout, mirrors and no mirrors
XE_FLOOR = dict(loss=1.3e-5, logp=9.5e-4, logp_rms=9.3e-5, cat=7.0e-4, grad_cos=7.1e-6)
# per parameter: the smallest rtol with which the float32 emulation passes grad_misses' max-norm bound against the float64 one
# ((max |f32 - f64| - atol) / max |f64|), worst of XE_CASES, flip-exempted rows left out.
# grad_misses' element-wise bound is left to the max-norm one (elem_share = 1): it gives an element a tenth of the max-norm bound
# plus a share of its own size, which fits errors that scale with the element; an operand that rounds the other way moves by 2^-8
# of ITS size and lands on whatever elements its products feed (the float32 emulation itself misses that bound on 8 - 29 parameters).
XE_ELEM_SHARE = 1.0
XE_GRAD_FLOOR = {
    "two_spatial_encoder.visual_emb_rgb.0.weight": 2.7e-03,
    "two_spatial_encoder.visual_emb_rgb.1.weight": 1.1e-03,
    "two_spatial_encoder.visual_emb_rgb.1.bias": 9.2e-04,
    "two_spatial_encoder.visual_emb_opfl.0.weight": 3.6e-03,
    "two_spatial_encoder.visual_emb_opfl.1.weight": 1.1e-03,
    "two_spatial_encoder.visual_emb_opfl.1.bias": 9.6e-04,
    "two_spatial_encoder.lstmcell_rgb.weight_ih": 1.4e-03,
    "two_spatial_encoder.lstmcell_rgb.weight_hh": 8.9e-04,
    "two_spatial_encoder.lstmcell_rgb.bias_ih": 8.1e-04,
    "two_spatial_encoder.lstmcell_rgb.bias_hh": 8.1e-04,
    "two_spatial_encoder.lstmcell_opfl.weight_ih": 1.6e-03,
    "two_spatial_encoder.lstmcell_opfl.weight_hh": 1.2e-03,
    "two_spatial_encoder.lstmcell_opfl.bias_ih": 1.0e-03,
    "two_spatial_encoder.lstmcell_opfl.bias_hh": 1.0e-03,
    "two_spatial_encoder.gate_rgb.gate.0.weight": 1.5e-03,
    "two_spatial_encoder.gate_rgb.gate.0.bias": 1.3e-03,
    "two_spatial_encoder.gate_opfl.gate.0.weight": 1.5e-03,
    "two_spatial_encoder.gate_opfl.gate.0.bias": 1.0e-03,
    "two_spatial_encoder.fusion.late_fusion.0.weight": 7.6e-04,
    "two_spatial_encoder.fusion.late_fusion.0.bias": 4.8e-04,
    "img_embed_h_1.weight": 1.8e-03,
    "img_embed_h_1.bias": 1.8e-03,
    "img_embed_c_1.weight": 7.9e-04,
    "img_embed_c_1.bias": 8.2e-04,
    "img_embed_h_2.weight": 1.0e-03,
    "img_embed_h_2.bias": 8.9e-04,
    "img_embed_c_2.weight": 1.6e-04,
    "img_embed_c_2.bias": 1.6e-04,
    "lstmcore.gate.gate.0.weight": 2.1e-03,
    "lstmcore.gate.gate.0.bias": 9.1e-04,
    "lstmcore.lstm_1.i2h.weight": 1.5e-03,
    "lstmcore.lstm_1.i2h.bias": 5.9e-04,
    "lstmcore.lstm_1.a2h.weight": 8.8e-04,
    "lstmcore.lstm_1.a2h.bias": 5.9e-04,
    "lstmcore.lstm_1.h2h.weight": 1.8e-03,
    "lstmcore.lstm_1.h2h.bias": 5.9e-04,
    "lstmcore.lstm_2.i2h.weight": 7.5e-04,
    "lstmcore.lstm_2.i2h.bias": 3.8e-04,
    "lstmcore.lstm_2.a2h.weight": 7.2e-04,
    "lstmcore.lstm_2.a2h.bias": 3.8e-04,
    "lstmcore.lstm_2.h2h.weight": 6.3e-04,
    "lstmcore.lstm_2.h2h.bias": 3.8e-04,
    "lstmcore.v2a.weight": 1.8e-03,
    "lstmcore.v2a.bias": 5.7e-04,
    "lstmcore.h2a.weight": 1.7e-03,
    "lstmcore.h2a.bias": 1.2e-03,
    "lstmcore.a2w.weight": 7.2e-04,
    "embed.weight": 1.5e-03,
    "logit.weight": 4.7e-04,
    "logit.bias": 9.9e-07,
    "classifer.0.weight": 1.1e-04,
    "classifer.0.bias": 8.4e-06,
    "classifer.3.weight": 6.2e-05,
    "classifer.3.bias": 2.0e-05,
}


def step_rtol(key):
    return bound(STEP_FLOOR[key], FP32_GRAD_RTOL, CAP_GRAD_RTOL)


# a tenth of the bf16 bound that stands beside each gradient (tests/test_gpu_fullsize.py: sampled elements within 3 % of the largest
# entry -- the issue of this test takes the 5 % of the norm bound --, 6 % for the two embedding matrices in front of train-mode
# BatchNorm, 12 % for the POS gate's bias: the cancellations named there)
XE_GRAD_CAP = {ENC + "visual_emb_rgb.0.weight": 6e-3, ENC + "visual_emb_opfl.0.weight": 6e-3, "lstmcore.gate.gate.0.bias": 1.2e-2}


def xe_grad_rtol(name):
    return bound(XE_GRAD_FLOOR[name], FP32_GRAD_RTOL, XE_GRAD_CAP.get(name, CAP_GRAD_RTOL))


# loss: today's bf16 bound is 1e-2, the floor 1e-5 -> the fp32 path's own 1e-4
XE_LOSS_TOL = bound(XE_FLOOR["loss"], FP32_LOSS_TOL, CAP_LOSS_TOL)
# log-probs: no whole-model bf16 test bounds them today (the rollout case allows 1e-2 on the gathered ones); the worst of 1.2 M
# elements is heavy-tailed (one operand of a 256-deep vocabulary product rounding the other way moves a whole row), so the
# largest element gets margin x floor as it is and the root mean square its own, much tighter, bound
XE_LOGP_TOL = FLOOR_MARGIN * XE_FLOOR["logp"]
XE_LOGP_RMS_TOL = FLOOR_MARGIN * XE_FLOOR["logp_rms"]
XE_CAT_TOL = FLOOR_MARGIN * XE_FLOOR["cat"]
XE_COS_MIN = 1.0 - bound(XE_FLOOR["grad_cos"], 1 - FP32_COS, 1 - CAP_COS)


def rel_cos(a, r):
    """(max |a - r| / max |r|, 1 - cosine) of two arrays"""
    a, r = np.asarray(a, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    scale = np.abs(r).max()
    na, nr = np.linalg.norm(a), np.linalg.norm(r)
    cos = float(a @ r / (na * nr)) if na > 0 and nr > 0 else 1.0
    return float(np.abs(a - r).max() / max(scale, 1e-300)), 1.0 - cos


# ---------------------------------------------------------------------------------------------------- stage 3: one decoder step
STEP_CASES = {
    # `mid`: everything 16-byte aligned -- the packed bf16 tiles (skf_kernel<., 1>) and, without them, sk_kernel<true, 1>
    "mid": dict(CFG["mid"]),
    # R a multiple of 8 (the skinny launcher takes the step) but E and A not multiples of 4, B no multiple of 32: the scalar-load
    # form sk_kernel<false, 1>
    "r8_unaligned": dict(B=5, K=3, R=24, A=38, E=10, V=37, C=3, L=4, F1=9, F2=7, H=128),
    # R, E, A not multiples of 8: the step goes out as plain GEMMs, which are far below the rule -- gemm_mode 1 rounds nothing here
    "odd": dict(CFG["odd"]),
}


def step_inputs(tag):
    """Seeded inputs of one decoder step (the set-up of test_single_step_backward_vs_oracle_autograd): float32 / int64 arrays."""
    d = pg.make_dims(**STEP_CASES[tag])
    B, K, R = d.B, d.K, d.R
    Pn = pg.make_params(d)
    x = dict(V=pg.uniform("sb.V", (B, K, R), 7, 0.0, 1.0), pos=pg.uniform("sb.pos", (B, R), 7, -1.0, 1.0),
             st=pg.uniform("sb.st", (4, B, R), 7, -0.5, 0.5), w=pg.uniform("sb.w", (4, B, R), 7, -1.0, 1.0),
             tok=pg.randint("sb.tok", (B,), 7, 2, d.V), mk=np.ones((B,), np.float32))
    x["mk"][min(2, B - 1)] = 0.0
    if B > 7:
        x["mk"][7] = 0.0
    # v2a(V) is an INPUT of the step: fp32 values, the same for the oracle and the kernel
    x["vproj"] = (x["V"].astype(np.float64) @ Pn["lstmcore.v2a.weight"].astype(np.float64).T + Pn["lstmcore.v2a.bias"]).astype(np.float32)
    return d, Pn, x


STEP_SKIP = ("lstmcore.a2w.bias", "lstmcore.v2a.weight", "lstmcore.v2a.bias")       # (not touched by a single step)


def step_oracle(tag, dtype=torch.float64, policy="hip"):
    """core_step under `policy` ("hip": hip_bf16_policy(d, "step"); None: plain) in `dtype`, loss = sum(new state * w).
    -> dict of float64 arrays: h1 c1 h2 c2 alpha, dstate (4,B,R), dV, dvproj, dpos, grads {name: array}."""
    d, Pn, x = step_inputs(tag)
    if policy == "hip":
        policy = hip_bf16_policy(d, "step")
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        P = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in Pn.items()}
        leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)      # noqa: E731
        Vt, vp, post = leaf(x["V"]), leaf(x["vproj"]), leaf(x["pos"])
        st = [leaf(x["st"][i]) for i in range(4)]
        xt = P["embed.weight"][torch.from_numpy(x["tok"])]
        _, ns, alpha = xo.core_step(P, xt, torch.from_numpy(x["mk"]).to(dtype).unsqueeze(1), Vt, post, [(st[0], st[1]), (st[2], st[3])],
                                    vproj=vp, policy=policy)
        wt = torch.from_numpy(x["w"]).to(dtype)
        loss = (ns[0][0] * wt[0]).sum() + (ns[0][1] * wt[1]).sum() + (ns[1][0] * wt[2]).sum() + (ns[1][1] * wt[3]).sum()
        loss.backward()
    finally:
        torch.set_default_dtype(old)
    f = lambda t: t.detach().double().numpy()           # noqa: E731
    out = dict(h1=f(ns[0][0]), c1=f(ns[0][1]), h2=f(ns[1][0]), c2=f(ns[1][1]), alpha=f(alpha),
               dstate=np.stack([f(s.grad) for s in st]), dV=f(Vt.grad), dvproj=f(vp.grad), dpos=f(post.grad))
    out["grads"] = {k: (f(v.grad) if v.grad is not None else np.zeros(tuple(v.shape)))
                    for k, v in P.items() if (k.startswith("lstmcore.") or k == "embed.weight") and k not in STEP_SKIP}
    return out


def step_floor(tag):
    """{quantity: max |f32 - f64| / max |f64|} of the emulated step, the gradients as one entry (their worst)"""
    a, b = step_oracle(tag, torch.float64), step_oracle(tag, torch.float32)
    out = {"state": max(rel_cos(b[k], a[k])[0] for k in ("h1", "c1", "h2", "c2")), "alpha": rel_cos(b["alpha"], a["alpha"])[0]}
    for k in ("dstate", "dV", "dvproj", "dpos"):
        out[k] = rel_cos(b[k], a[k])[0]
    out["grads"] = max(rel_cos(b["grads"][k], a["grads"][k])[0] for k in a["grads"])
    return out


# ---------------------------------------------------------------------------------------------------- stage 4: teacher-forced XE
# From test_scst_paired_rollout_bf16_mirrors_survive_the_compaction (B K >= 256, T B >= 256, pitches multiples of 8), with
#   B = 28: each HALF of the vocabulary forward (10 and 11 steps) has >= 256 rows, so that product rounds too (16 x 10 = 160 rows
#           would leave it in fp32), and 28 rows are no multiple of the 32-row tile
#   F1 = 256: the first modality's embedding product rounds; F2 = 64: the second one's forward stays fp32 (K < 256)
XE_DIMS = dict(B=28, K=20, R=256, A=384, E=64, V=2000, C=14, L=20, F1=256, F2=64)
XE_SEED = 90210                        # dropout seed of the p = 0.5 case
# which side of the rule each product is on at XE_DIMS (asserted by the tests: a change of dims cannot silently move them)
XE_FP32_SIDE = [(ENC + "visual_emb_opfl.0", "fwd"), ("lstmcore.gate.gate.0", "fwd"), ("lstmcore.lstm_1.i2h", "fwd"),
                ("classifer.0", "dx"), ("classifer.0", "dw"), ("classifer.3", "fwd"), ("classifer.3", "dx"), ("classifer.3", "dw"),
                ("img_embed_h_1", "dw"), ("img_embed_c_1", "dw"), ("img_embed_h_2", "dw"), ("img_embed_c_2", "dw")]


# ReLU sites behind a ROUNDED product of COMPUTED operands (cross gates, fusion, classifier hidden): an operand that rounds the other
# way moves such a pre-activation by ~1e-4, thirty of 500 000 then change sign between the float32 and the float64 emulation, and one
# flipped derivative moves every gradient upstream of it by up to 9e-3 of its scale (measured with the seeded biases) -- above the
# condition on the floor (5e-3).  The biases of these four sites are shifted so that their pre-activations (standard deviation
# 0.1-0.2) stay clear of zero: this test is about the roundings; the ReLU sites have their own (tests/util.py: flip_exemptions).
XE_RELU_BIAS_SHIFT = {ENC + "gate_rgb.gate.0.bias": 1.0, ENC + "gate_opfl.gate.0.bias": 1.0, "classifer.0.bias": 1.0,
                      # (the fusion's output is V: a large constant in every V[b, k] makes the attention's gradients cancel even more)
                      ENC + "fusion.late_fusion.0.bias": 0.7}
# The seeded features are i.i.d. over the frames, so the encoder's outputs of one video are nearly the same at every frame and the
# attention's gradients cancel across them: lstmcore.v2a.weight (sum over frames of dvproj^T V, with sum_k dvproj[b, k] ~ 0) then
# has a floor of 7e-3.  The frames get distinct scales (rgb rising, optical flow falling), which train-mode BatchNorm keeps.
XE_FRAME_RAMP = (0.1, 1.9)


# the stage-4 cases: (ragged, drop_prob_lm, workspace with a mirror region)
# (dropout on the dense captions: under a ragged mask the held rows of a finished caption go through dropout again at every step,
#  x 2 or x 0 each time, and what the log-probs hold there -- outside the loss -- is round-off amplified by 2^steps)
XE_CASES = [(False, 0.0, True), (True, 0.0, True), (False, 0.5, True), (True, 0.0, False)]


# The loss is a mean over T B positions and the gradients of this shape are 1e-5 .. 1e-2 at their largest: the absolute part of the
# gradient bound (2e-6, the fp32 path's own) would be a fifth of the smallest scale.  The loss is multiplied by a power of two
# (exact in every format), after which the absolute part is below 2e-4 of every parameter's scale.
XE_LOSS_GAIN = 1024.0


def xe_dims():
    return pg.make_dims(**XE_DIMS)


def xe_expected_sides(d):
    """Every product rounds at XE_DIMS except XE_FP32_SIDE, a2w, and the directions that do not exist."""
    tab = policy_table(d, "xe")
    none = {k for k in tab if tab[k][4] in ("attention kernels: fp32", "no gradient wrt the features", "vbar is detached", "own fp32 pass", "-")}
    for key, (M, N, K, rounds, why) in tab.items():
        if key in none or key[1] in ("val", "grad"):
            continue
        assert rounds == (key not in XE_FP32_SIDE), (key, M, N, K, rounds)
    return tab


def xe_case(ragged, p):
    d = xe_dims()
    Pn = pg.make_params(d, logit_gain=1.0)
    for name, shift in XE_RELU_BIAS_SHIFT.items():
        Pn[name] = Pn[name] + np.float32(shift)
    xn = pg.make_inputs(d, seed=0, ragged=ragged)
    ramp = (XE_FRAME_RAMP[0] + (XE_FRAME_RAMP[1] - XE_FRAME_RAMP[0]) * np.arange(d.K, dtype=np.float32) / (d.K - 1))[None, :, None]
    xn["feats_rgb"] = xn["feats_rgb"] * ramp
    xn["feats_opfl"] = xn["feats_opfl"] * ramp[:, ::-1]
    return d, Pn, xn


def xe_fn(d, p, policy, weight_class=WEIGHT_CLASS):
    """run_oracle's fn: forward_xe + both criteria under `policy`; extra = (logp, cat, l_xe, l_cls)"""
    def fn(P, xi, tr):
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"], xi["seq_mask"],
                                     train=True, p=p, seed=XE_SEED, running=xo.new_running(d), relu_trace=tr, policy=policy)
        l_xe = xo.lm_criterion(logp, xi["seq"], xi["seq_mask"])
        l_cls = xo.cls_criterion(cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"])
        return XE_LOSS_GAIN * (l_xe + weight_class * l_cls), (logp.detach().double().numpy(), cat.detach().double().numpy(), l_xe.item(), l_cls.item())
    return fn


@functools.lru_cache(maxsize=None)
def xe_oracle(ragged, p, mirrors=True, omit=()):
    """The emulated oracle of one stage-4 case in float64 and float32 (computed once per process, shared; treat as read-only).
    -> dict(loss, logp, cat, l_xe, l_cls, grads) of the float64 run, f32 = the same of the float32 run, exempt = flip_exemptions."""
    d, Pn, xn = xe_case(ragged, p)
    policy = hip_bf16_policy(d, "xe", mirrors=mirrors, omit=omit)
    fn = xe_fn(d, p, policy)
    out = {}
    traces = {}
    for key, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        loss, (logp, cat, l_xe, l_cls), grads, traces[key] = run_oracle(Pn, xn, fn, dtype)
        out[key] = dict(loss=loss, logp=logp, cat=cat, l_xe=l_xe, l_cls=l_cls, grads=grads)
    res = dict(out["f64"], f32=out["f32"], d=d, Pn=Pn, xn=xn)
    res["counts"] = {}
    res["exempt"] = flip_exemptions(traces["f64"], traces["f32"], {k: v.shape for k, v in Pn.items()}, counts=res["counts"])
    return res


def xe_floor(ref):
    """Floors of one xe_oracle result: dict(loss, logp, logp_rms, cat, grads={name: (rel, 1 - cos)}) -- the flip-exempted elements
    left out; rel = the smallest rtol with which the float32 run passes grad_misses' max-norm bound"""
    f = ref["f32"]
    out = dict(loss=max(abs(f["l_xe"] - ref["l_xe"]), abs(f["l_cls"] - ref["l_cls"])),
               logp=float(np.abs(f["logp"] - ref["logp"]).max()), cat=float(np.abs(f["cat"] - ref["cat"]).max()),
               logp_rms=float(np.sqrt(((f["logp"] - ref["logp"]) ** 2).mean())), grads={})
    for name, r in ref["grads"].items():
        if name in ZERO_GRAD_PARAMS:
            continue
        keep = ~ref["exempt"][name] if name in ref["exempt"] else np.ones(r.shape, bool)
        scale = np.abs(r).max()
        if not keep.any():
            continue
        rel, c = rel_cos(f["grads"][name][keep], r[keep])
        # grad_misses (1): |g - r| <= atol + rtol scale -- the smallest rtol that holds
        err = np.abs(f["grads"][name][keep] - r[keep]) - FP32_GRAD_ATOL
        out["grads"][name] = (max(0.0, float(err.max() / scale)), c)
    return out
