"""The GEMM planner (csrc/xg_gemm_route.h: xg_gemm_plan) on the CPU: tools/gemm_route_dump.cc, compiled here with g++, against the
recorded table tests/golden/gemm_routes.json (tools/gen_gemm_routes_golden.py) -- which kernel, tile, split, grid, LDS and side work
every shape of tests/gemm_shapes.py gets.  A routing change shows as a diff of that table; nothing here needs a GPU."""
import json
import subprocess

import pytest

from tests import bf16_oracle as bo
from tests import gemm_shapes as gs
from tools import gen_gemm_routes_golden as gen

WIDE = ("gemm_bs1", "gemm_bs3", "gemm_bx", "g16")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return gen.build_dump(tmp_path_factory.mktemp("gemm_route_dump"))


@pytest.fixture(scope="module")
def golden():
    with open(gen.PATH) as f:
        return json.load(f)


def _families(golden, inputs):
    fi = golden["keys"].index("family")
    return [golden["routes"][gs.key(e)][fi] for e in inputs]


def test_every_recorded_route_is_reproduced(dump, golden):
    now = gen.table(dump)
    assert now["keys"] == golden["keys"]
    assert list(now["routes"]) == list(golden["routes"]), "tests/gemm_shapes.table_inputs() and the recorded table list different shapes"
    diff = {k: (golden["routes"][k], v) for k, v in now["routes"].items() if golden["routes"][k] != v}
    assert not diff, "routes changed (recorded, now): %s" % json.dumps(dict(list(diff.items())[:8]))


def test_bf16_oracle_rule_is_the_planners_floor(dump):
    """tests/bf16_oracle.rule(M, N, K) is true exactly where the planner leaves the fp32 family in modes 1 and 3 with transA false
    (default XG_X3_FP32), for every shape of the table."""
    shapes = sorted({(e["M"], e["N"], e["K"]) for e in gs.table_inputs()})
    inputs = [dict(mode=mode, ta=0, tb=tb, M=M, N=N, K=K) for M, N, K in shapes for mode in (1, 3) for tb in (0, 1)]
    for e, r in zip(inputs, gen.routes(dump, inputs)):
        assert r["rc"] == 0 and (r["family"] in WIDE) == bo.rule(e["M"], e["N"], e["K"]), (e, r["family"])


def test_table_covers_every_family_and_one_round_tile(dump, golden):
    keys = golden["keys"]
    rows = list(golden["routes"].values())
    assert {r[keys.index("family")] for r in rows} >= set(gs.FAMILIES)
    tiles = json.loads(subprocess.run([dump, "--w1-tiles"], check=True, capture_output=True, text=True).stdout)
    assert len(tiles) == 8
    seen = {(r[keys.index("bm")], r[keys.index("bn")], r[keys.index("bk")]) for r in rows if r[keys.index("family")] == "gemm_w1"}
    assert seen == {tuple(t) for t in tiles}


VARIANTS = 462          # of the recorded table; a smaller number is coverage lost: tests/test_gpu_gemm_variants.py runs one input of each
VARIANTS_PER_FAMILY = {"gemm_kernel": 147, "gemm_w1": 67, "gemm_bs1": 69, "gemm_bs3": 56, "g16": 47, "gemm_pk": 43, "gemm_td": 18,
                       "gemm_bx": 14, "none": 1}      # (none: the one refused input)


def test_variant_cases_cover_the_table_within_a_budget(golden):
    """tests/gemm_shapes.variant_cases: one input per variant, every variant of the table, each within 70 G multiply-adds (M N K;
    the largest is 4096^3 in mode 3) and 3 GiB of operands, 2 T multiply-adds together -- what tests/test_gpu_gemm_variants.py runs
    on the GPU, with a float64 product beside each.  Every family that fuses the column sums runs them into 1, 2 and 3 accumulators."""
    cases = gs.variant_cases(golden)
    keys = golden["keys"]
    all_variants = {gs.variant(e, dict(zip(keys, golden["routes"][gs.key(e)]))) for e in gs.table_inputs()}
    assert set(cases) == all_variants
    assert len(cases) == VARIANTS
    per = {}
    for v in cases:
        per[v[1]] = per.get(v[1], 0) + 1
    assert per == VARIANTS_PER_FAMILY
    for v, e in cases.items():
        assert gs.variant(e, dict(zip(keys, golden["routes"][gs.key(e)]))) == v
        rows = (e["K"] if e["ta"] else e["M"], e["N"] if e["tb"] else e["K"], e["M"])
        pitch = [e.get(k, 0) or n for k, n in zip(("lda", "ldb", "ldc"), gs.row_lengths(e))]
        assert e["M"] * e["N"] * e["K"] <= 70e9, gs.key(e)
        assert 4 * sum(r * p for r, p in zip(rows, pitch)) <= 3 << 30, gs.key(e)
    assert sum(e["M"] * e["N"] * e["K"] for e in cases.values()) <= 2e12
    f = gs.VARIANT_FIELDS.index
    fused = {}
    for v in cases:
        if v[f("colsum")] == 1:      # XGR_CS_FUSED
            fused.setdefault(v[f("family")], set()).add(v[f("ncs")])
    assert set(fused) == {"gemm_kernel", "gemm_pk", "gemm_td", "gemm_bs1", "gemm_bs3", "g16"}
    assert all(n == {1, 2, 3} for n in fused.values()), fused
    assert any(v[f("colsum")] == 2 and v[f("ncs")] == 3 for v in cases)      # ... and the separate pass
    for fam in ("gemm_bs1", "gemm_bs3"):      # gemm_bs_kernel sums per load width: one row (scalar loads) and four (16-byte loads)
        assert {(v[f("vec")], v[f("ncs")]) for v in cases if v[f("family")] == fam and v[f("ncs")]} == {(x, n) for x in (0, 1) for n in (1, 2, 3)}


def test_pitched_inputs_start_from_the_cheapest_shape_of_every_family(dump):
    """tests/gemm_shapes.CHEAPEST is what the `cheapest` fixture of tests/test_gpu_gemm_routes.py finds"""
    shapes = sorted(set(gs.LAYOUTS + gs.PERSISTENT + gs.BF16_OPERANDS + gs.BF16_MODES + list(gs.W1_SHAPES) + list(gs.TD_SHAPES) +
                        [s[:3] for s in gs.BG_SMALL_M] + [s[3:6] for s in gs.GEMM_BENCH]), key=lambda s: (s[0] * s[1] * s[2], s))
    cases = [(entry, bias, s, l) for s in shapes for entry in gs.ENTRY_INPUTS for bias in (1, 0) for l in gs.LAYOUT_CASES]
    inputs = [dict(gs.ENTRY_INPUTS[entry], ta=l[0], tb=l[1], M=s[0], N=s[1], K=s[2], bias=bias) for entry, bias, s, l in cases]
    best = {}
    for (entry, bias, s, l), r in zip(cases, gen.routes(dump, inputs)):
        pick = best.setdefault(r["family"], (entry, bias, s, []))
        if pick[:3] == (entry, bias, s):
            pick[3].append(l)
    assert best == gs.CHEAPEST


def test_planned_product_entry_is_in_the_diag_library_only():
    import ctypes as C
    import __graft_entry__ as ge
    from controllable_xgating_amd import _native as nv
    ge.build()
    assert hasattr(C.CDLL(nv.LIB_DIAG_PATH), "xg_debug_gemm_planned")
    assert not hasattr(C.CDLL(nv.LIB_PATH), "xg_debug_gemm_planned")


def test_existing_gpu_tests_reach_every_family(golden):
    """each kernel family is launched by at least one shape of the GPU GEMM tests (under the switches those tests set)"""
    srcs = {k: v for k, v in gs.gpu_test_inputs().items() if k.startswith("test_")}
    reached = {f for v in srcs.values() for f in _families(golden, v)}
    assert reached >= set(gs.FAMILIES), set(gs.FAMILIES) - reached
