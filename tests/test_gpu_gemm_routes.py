"""A kernel family the GEMM planner names is one the launchers can launch: for every family, the cheapest shape of
tests/gemm_shapes.py that the planner (csrc/xg_gemm_route.h, default tuning) sends there, in every layout in which it does,
through the product library against a float64 product.  Tolerances: those of test_gemm_layouts (fp32, and bf16 operands that ARE
the bf16 values) and test_gemm_bf16_modes (split-bf16 4e-6, bf16 2e-2, relative to max |C|)."""
import numpy as np
import pytest
import torch

from tests import gemm_shapes as gs
from tools import gen_gemm_routes_golden as gen

pytestmark = pytest.mark.gpu

ENTRIES = {"xg_gemm": dict(mode=0), "xg_gemm_mode_3": dict(mode=3, wide=1), "xg_gemm_mode_1": dict(mode=1, wide=1),
           "xg_gemm_bf16_operands": dict(mode=1, wide=1, a16=1, b16=1)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(scope="module")
def cheapest(tmp_path_factory):
    """{family: (entry, bias, (M, N, K), [(ta, tb) the planner routes there])} with the fewest flops per family"""
    exe = gen.build_dump(tmp_path_factory.mktemp("gemm_route_dump"))
    shapes = sorted(set(gs.LAYOUTS + gs.PERSISTENT + gs.BF16_OPERANDS + gs.BF16_MODES + list(gs.W1_SHAPES) + list(gs.TD_SHAPES) +
                        [s[:3] for s in gs.BG_SMALL_M] + [s[3:6] for s in gs.GEMM_BENCH]), key=lambda s: (s[0] * s[1] * s[2], s))
    cases = [(entry, bias, s, l) for s in shapes for entry in ENTRIES for bias in (1, 0) for l in gs.LAYOUT_CASES]
    inputs = [dict(ENTRIES[entry], ta=l[0], tb=l[1], M=s[0], N=s[1], K=s[2], bias=bias) for entry, bias, s, l in cases]
    best = {}
    for (entry, bias, s, l), r in zip(cases, gen.routes(exe, inputs)):
        assert r["rc"] == 0
        pick = best.setdefault(r["family"], (entry, bias, s, []))
        if pick[:3] == (entry, bias, s):
            pick[3].append(l)
    return best


@pytest.mark.parametrize("family", gs.FAMILIES)
def test_planned_family_runs_and_matches_float64(family, cheapest):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    assert family in cheapest, "no shape of tests/gemm_shapes.py reaches " + family
    entry, has_bias, (M, N, K), layouts = cheapest[family]
    print(family, entry, "bias" if has_bias else "no bias", (M, N, K), layouts)
    for ta, tb in layouts:
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K + ta * 2 + tb)
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        Bm = torch.randn((N, K) if tb else (K, N), generator=g)
        if entry == "xg_gemm_bf16_operands":
            A, Bm = A.bfloat16(), Bm.bfloat16()
        bias = torch.randn(N, generator=g)
        C0 = torch.randn(M, N, generator=g)
        ref = (A.t() if ta else A).double() @ (Bm.t() if tb else Bm).double() + (bias.double() if has_bias else 0)
        A16, B16, bd = A.cuda(), Bm.cuda(), bias.cuda()
        Ad, Bd = A16.float(), B16.float()
        bp = nv.ptr(bd) if has_bias else None
        for relu, acc in gs.EPILOGUES:      # (the family is the plain store's; ReLU / += C may route elsewhere: that must run too)
            Cd = C0.clone().cuda()
            if entry == "xg_gemm":
                rc = L.xg_gemm(None, ta, tb, M, N, K, nv.ptr(Ad), A.shape[1], nv.ptr(Bd), Bm.shape[1], nv.ptr(Cd), N, bp, relu, acc)
            elif entry == "xg_gemm_bf16_operands":
                rc = L.xg_gemm_bf16_operands(None, ta, tb, M, N, K, nv.ptr(Ad), nv.ptr(A16), A.shape[1], nv.ptr(Bd), nv.ptr(B16), Bm.shape[1],
                                             nv.ptr(Cd), N, bp, relu, acc)
            else:
                rc = L.xg_gemm_mode(None, ENTRIES[entry]["mode"], ta, tb, M, N, K, nv.ptr(Ad), A.shape[1], nv.ptr(Bd), Bm.shape[1], nv.ptr(Cd), N,
                                    bp, relu, acc)
            assert rc == 0
            want = ref + (C0.double() if acc else 0)
            if relu:
                want = want.clamp(min=0)
            err = float((Cd.cpu().double() - want).abs().max())
            scale = float(want.abs().max())
            if entry in ("xg_gemm", "xg_gemm_bf16_operands"):
                assert err <= (2e-6 * np.sqrt(K) * 4 + 1e-6) * max(1.0, scale), (ta, tb, relu, acc, err)
            else:
                assert err / scale < (4e-6 if entry == "xg_gemm_mode_3" else 2e-2), (ta, tb, relu, acc, err / scale)
