"""The bf16-rounding oracle (oracle/xgate_oracle.py: _mm / rb, tests/bf16_oracle.py: hip_bf16_policy) on the CPU: the rounding
rule, the hook itself, the floor the GPU bounds are derived from, and that those bounds see planted errors which today's bf16
bounds (5 % of the norm, cosine 0.997) let through."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import bf16_oracle as bo
from tests.util import ZERO_GRAD_PARAMS, grad_misses, run_oracle


# ---------------------------------------------------------------------------------------------------- the rounding rule
def _grid():
    """fp32 bit patterns around bf16 rounding boundaries: exact ties above an even and above an odd bf16 value, one fp32 ulp either
    side of each, both signs, in the normal range, in the fp32 / bf16 denormal range, +-0 and the largest finite bf16."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x00FF, 0x0080, 0x0001, 0x0002, 0x0000, 0x7F7E, 0x7F00):      # upper 16 bits (bf16 patterns)
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):                                    # tie = 0x8000
            bits.append((hi << 16) | lo)
    bits.append(0x7F7F0000)                                                                            # largest finite bf16
    bits.append(0x7F7F7FFF)                                                                            # just below its upper tie
    b = np.array(bits, np.uint32)
    return np.concatenate([b, b | np.uint32(0x80000000)]).view(np.float32)


def test_rb_is_round_to_nearest_even_of_the_fp32_value():
    """rb == tensor.float().to(torch.bfloat16): ties go to the even bf16 value in both directions, one ulp either side of a tie goes
    to its side, denormals keep their bits' rounding, zeros keep their sign.  The kernels' rule: csrc/xg_step.hip:88-92 (bf16_rne,
    the same integer form as rb) and :96 / csrc/xg_gemm_bf16.hip:594-604 (the __bf16 cast, v_cvt_pk_bf16_f32: RNE)."""
    x = torch.from_numpy(_grid().copy())
    want = x.to(torch.bfloat16).to(torch.float32)
    got = xo.rb(x)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    # the two directions of a tie, spelled out: 1 + 2^-8 is halfway between 1 (even) and 1 + 2^-7; 1 + 3 * 2^-8 between odd and even
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)])
    assert xo.rb(t).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6)]
    # a float64 value goes through fp32 first: 1 + 2^-8 + 2^-40 is above the tie in float64 but IS the tie in fp32
    d = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    assert xo.rb(d).dtype == torch.float64 and xo.rb(d).tolist() == [1.0, 1 + 2.0 ** -7]
    # seeded values of ordinary size
    r = torch.from_numpy(pg.uniform("rb.grid", (4096,), 3, -3.0, 3.0))
    assert torch.equal(xo.rb(r), r.to(torch.bfloat16).to(torch.float32))


# ---------------------------------------------------------------------------------------------------- the hook
def _toy():
    x = torch.from_numpy(pg.uniform("mm.x", (3, 5, 8), 1, -1, 1)).double().requires_grad_(True)
    W = torch.from_numpy(pg.uniform("mm.w", (6, 8), 1, -1, 1)).double().requires_grad_(True)
    b = torch.from_numpy(pg.uniform("mm.b", (6,), 1, -1, 1)).double().requires_grad_(True)
    dy = torch.from_numpy(pg.uniform("mm.dy", (3, 5, 6), 1, -1, 1)).double()
    return x, W, b, dy


@pytest.mark.parametrize("on", [(), ("fwd",), ("dx",), ("dw",), ("db",), ("fwd", "dx", "dw", "db")])
def test_mm_rounds_exactly_what_the_policy_switches_on(on):
    """_mm under a policy: forward rb(x) rb(W)^T, dx = rb(dy) rb(W), dW = rb(dy)^T rb(x), db = sum rb(dy) -- each on its own switch,
    the kernel-side extents handed to the policy (rows x out x in, rows x in x out, out x in x rows); nothing switched on is the
    plain product and its plain gradients; no policy is the very expression the oracle had before."""
    x, W, b, dy = _toy()
    seen = {}

    def policy(site, kind, M, N, K):
        seen[kind] = (site, M, N, K)
        return kind in on

    y = xo._mm(x, W, "toy", policy, b)
    y.backward(dy)
    assert seen == {"fwd": ("toy", 15, 6, 8), "dx": ("toy", 15, 8, 6), "dw": ("toy", 6, 8, 15), "db": ("toy", 6, 8, 15)}
    rb = xo.rb
    xd, Wd, d2 = x.detach(), W.detach(), dy.reshape(-1, 6)
    f = (lambda t: rb(t)) if "fwd" in on else (lambda t: t)
    assert torch.equal(y.detach(), f(xd) @ f(Wd).t() + b.detach())
    assert torch.equal(x.grad, (rb(dy) @ rb(Wd)) if "dx" in on else dy @ Wd)
    assert torch.equal(W.grad, (rb(d2).t() @ rb(xd).reshape(-1, 8)) if "dw" in on else d2.t() @ xd.reshape(-1, 8))
    assert torch.equal(b.grad, (rb(d2) if "db" in on else d2).sum(0))
    plain = xo._mm(xd, Wd, "toy", None, b.detach())
    assert torch.equal(plain, xd @ Wd.t() + b.detach())
    if not on:
        assert torch.equal(y.detach(), plain)


def test_round_point_switches_value_and_gradient():
    x = torch.from_numpy(pg.uniform("rp.x", (4, 7), 2, -1, 1)).double().requires_grad_(True)
    dy = torch.from_numpy(pg.uniform("rp.dy", (4, 7), 2, -1, 1)).double()
    assert xo._rpoint(x, "s", None) is x
    for val, grad in ((False, False), (True, False), (False, True)):
        x.grad = None
        y = xo._rpoint(x, "s", lambda site, kind, M, N, K: {"val": val, "grad": grad}[kind])
        y.backward(dy)
        assert torch.equal(y.detach(), xo.rb(x.detach()) if val else x.detach())
        assert torch.equal(x.grad, xo.rb(dy) if grad else dy)


def test_policy_knows_every_site_of_the_oracle_and_nothing_else():
    """forward_xe + both criteria under a recording policy at a tiny shape: the sites the oracle asks about are exactly the sites
    of policy_table (a product added to the oracle has to be entered there; an entry nobody asks about is stale)."""
    d = pg.make_dims(**bo.CFG["tiny"])
    asked = set()
    real = bo.hip_bf16_policy(d, "xe")

    def policy(site, kind, M, N, K):
        asked.add((site, kind))
        return real(site, kind, M, N, K)

    run_oracle(pg.make_params(d), pg.make_inputs(d, seed=0, ragged=True), bo.xe_fn(d, 0.0, policy), torch.float64)
    assert asked == set(bo.policy_table(d, "xe"))
    assert bo.rounding_sites(d, "xe") and all(bo.policy_table(d, "xe")[k][4] == "step" for k in bo.rounding_sites(d, "xe"))
    assert not bo.rounding_sites(pg.make_dims(**dict(bo.CFG["tiny"], R=22)), "xe")      # tiny and R % 4 != 0: gemm_mode 1 rounds nothing


def test_xe_dims_are_on_both_sides_of_the_rule():
    tab = bo.xe_expected_sides(bo.xe_dims())
    assert sum(v[3] for v in tab.values()) > 50 and all(not tab[k][3] for k in bo.XE_FP32_SIDE)


# ---------------------------------------------------------------------------------------------------- the floor
def test_floor_of_the_decoder_step_is_fp32_class():
    """Stage 3: one step has too few computed operands for one to sit on a rounding boundary -- the float32 and the float64
    emulation agree to fp32 round-off, so the step's bounds are the fp32 path's own (2e-3 / 2e-6)."""
    for tag in bo.STEP_CASES:
        fl = bo.step_floor(tag)
        print("step floor", tag, {k: "%.1e" % v for k, v in fl.items()})
        for k, v in fl.items():
            assert v <= 2 * bo.STEP_FLOOR[k] + 1e-7, (tag, k, v)
            assert bo.step_rtol(k) == bo.FP32_GRAD_RTOL


def test_floor_of_the_xe_cases_meets_the_condition_and_the_recorded_constants():
    """Stage 4: the float32 emulation against the float64 one on every case of XE_CASES.  The condition on the inputs: every
    gradient's floor at most 5e-3 of its scale and the loss's at most 1e-3 (a tenth of today's bf16 bounds) -- otherwise the
    bounds derived from it would buy nothing.  And the constants in tests/bf16_oracle.py are these floors (a recorded one may be
    up to twice too small before this fails: float32 BLAS results, and with them which operands round the other way, differ a
    little between machines)."""
    worst = {}
    for case in bo.XE_CASES:
        fl = bo.xe_floor(bo.xe_oracle(*case))
        print("xe floor", case, {k: "%.2e" % fl[k] for k in ("loss", "logp", "logp_rms", "cat")},
              "grad max %.2e, 1 - cos max %.1e" % (max(r for r, _ in fl["grads"].values()), max(c for _, c in fl["grads"].values())))
        assert fl["loss"] <= 1e-3
        for k in ("loss", "logp", "logp_rms", "cat"):
            assert fl[k] <= 2 * bo.XE_FLOOR[k], (case, k, fl[k])
        for name, (rel, c) in fl["grads"].items():
            assert rel <= 5e-3, (case, name, rel)
            assert rel <= 2 * bo.XE_GRAD_FLOOR[name] + 5e-4, (case, name, rel, bo.XE_GRAD_FLOOR[name])
            assert c <= 2 * bo.XE_FLOOR["grad_cos"], (case, name, c)
            worst[name] = max(worst.get(name, 0.0), rel)
    assert set(worst) == set(bo.XE_GRAD_FLOOR) and not set(worst) & set(ZERO_GRAD_PARAMS)
    for name in worst:       # every bound: margin x floor inside [fp32 path's own, a tenth of the bf16 bound beside it]
        assert bo.FP32_GRAD_RTOL <= bo.xe_grad_rtol(name) <= bo.XE_GRAD_CAP.get(name, bo.CAP_GRAD_RTOL)
    assert bo.XE_LOSS_TOL == bo.FP32_LOSS_TOL and bo.XE_COS_MIN >= bo.CAP_COS


# ---------------------------------------------------------------------------------------------------- discrimination
def _new_bound_misses(g, ref):
    bad = []
    for name in ref["grads"]:
        if name not in ZERO_GRAD_PARAMS:
            bad += grad_misses({name: g[name]}, ref["grads"], rtol=bo.xe_grad_rtol(name), atol=bo.FP32_GRAD_ATOL, cos_min=bo.XE_COS_MIN,
                               exempt=ref["exempt"], elem_share=bo.XE_ELEM_SHARE)
    return bad


def _old_bounds_pass(g, ref):
    """today's bf16 bounds (tests/test_gpu_fullsize.py): every gradient norm within 5 %, cosine at least 0.997"""
    for name, r in ref["grads"].items():
        if name in ZERO_GRAD_PARAMS:
            continue
        gn, rn = np.linalg.norm(g[name]), np.linalg.norm(r)
        if not abs(gn - rn) <= 5e-2 * rn + 1e-6 or not float(g[name].ravel() @ r.ravel()) / (gn * rn) >= 0.997:
            return False
    return True


W_RGB = bo.ENC + "visual_emb_rgb.0.weight"
MUTATIONS = {
    # one forward product reads its fp32 operands where the kernel reads rounded ones
    "forward_rounding_omitted": dict(omit=((bo.ENC + "visual_emb_rgb.0", "fwd"),), fed={W_RGB}),
    # one weight-gradient product converts its operands by truncation (a conversion without the rounding increment): every term
    # shrinks by ~2^-8, coherently -- 0.55 % of the norm
    "dw_conversion_truncates": dict(truncate=(("lstmcore.lstm_2.a2h", "dw"),), fed={"lstmcore.lstm_2.a2h.weight"}),
    # one 32 x 32 tile of one weight gradient off by 1 % of its largest entry
    "wrong_tile": dict(tile=("lstmcore.lstm_2.i2h.weight", slice(64, 96), slice(128, 160)), fed={"lstmcore.lstm_2.i2h.weight"}),
}


@pytest.mark.parametrize("kind", sorted(MUTATIONS))
def test_planted_error_misses_the_new_bound_and_passes_todays(kind):
    """The ragged stage-4 case with one planted error each: the float64 run of a mutated policy (one forward product that rounds
    nothing; one weight-gradient product that truncates), or one wrong tile.  The stage-4 bound misses on the parameters the error
    feeds; today's bf16 bounds pass all three -- as they pass the unmutated float32 emulation, which the new bound passes too."""
    m = MUTATIONS[kind]
    ref = bo.xe_oracle(True, 0.0, True)
    assert _new_bound_misses(ref["f32"]["grads"], ref) == [] and _old_bounds_pass(ref["f32"]["grads"], ref)
    if "tile" not in m:
        d, Pn, xn = bo.xe_case(True, 0.0)
        policy = bo.hip_bf16_policy(d, "xe", omit=m.get("omit", ()), truncate=m.get("truncate", ()))
        _, _, g, _ = run_oracle(Pn, xn, bo.xe_fn(d, 0.0, policy), torch.float64)
    else:
        name, rows, cols = m["tile"]
        g = {k: v.copy() for k, v in ref["grads"].items()}
        g[name][rows, cols] += 0.01 * np.abs(g[name]).max()
    bad = _new_bound_misses(g, ref)
    print(kind, bad)
    assert {b[0] for b in bad} >= m["fed"], bad
    assert _old_bounds_pass(g, ref)


def test_one_omitted_dw_rounding_is_inside_the_floor():
    """What the new bound does NOT see, measured: a weight-gradient product that rounds NOTHING where the kernel rounds.  Its terms
    change by ~2^-9 of their size with random sign and average out over the 560 - 588 rows of the product: 0.3e-3 .. 3.8e-3 of the
    scale over the 19 weight-gradient sites (lstmcore.v2a, the largest, here), which is the size of the floor itself -- no bound that
    leaves FLOOR_MARGIN times the floor can tell it from an operand that rounds the other way.  (In the kernels the case does not
    arise as such: a product that reads the fp32 operand instead of its mirror converts it on the fly to the same bf16 value.)"""
    ref = bo.xe_oracle(True, 0.0, True)
    d, Pn, xn = bo.xe_case(True, 0.0)
    _, _, g, _ = run_oracle(Pn, xn, bo.xe_fn(d, 0.0, bo.hip_bf16_policy(d, "xe", omit=(("lstmcore.v2a", "dw"),))), torch.float64)
    rel = bo.rel_cos(g["lstmcore.v2a.weight"], ref["grads"]["lstmcore.v2a.weight"])[0]
    print("v2a dw rounding omitted: %.2e of the scale, floor %.1e" % (rel, bo.XE_GRAD_FLOOR["lstmcore.v2a.weight"]))
    assert 1e-3 < rel < bo.FLOOR_MARGIN * bo.XE_GRAD_FLOOR["lstmcore.v2a.weight"]
    assert all(np.array_equal(g[k], v) for k, v in ref["grads"].items() if k != "lstmcore.v2a.weight")
