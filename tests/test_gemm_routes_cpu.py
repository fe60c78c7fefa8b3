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


def test_existing_gpu_tests_reach_every_family(golden):
    """each kernel family is launched by at least one shape of the GPU GEMM tests (under the switches those tests set)"""
    srcs = {k: v for k, v in gs.gpu_test_inputs().items() if k.startswith("test_")}
    reached = {f for v in srcs.values() for f in _families(golden, v)}
    assert reached >= set(gs.FAMILIES), set(gs.FAMILIES) - reached
