"""The checks of tests/gemm_variant_run.py themselves, without a GPU: a launcher written in torch that computes the product exactly
passes every small case of the table, and launchers that are wrong the way a kernel can be wrong -- a store into the pitch gap or
past the last row, a clamped edge row in the column sums, a poisoned element let into the reduction, a bias lost on the last
column, an operand written, a different route, work done for a refused input -- are each reported."""
import pytest

from tests import gemm_shapes as gs
from tests import gemm_variant_run as gv
from tools import gen_gemm_routes_golden as gen


@pytest.fixture(scope="module")
def golden():
    return gv.golden_table()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return gen.build_dump(tmp_path_factory.mktemp("gemm_route_dump"))


@pytest.fixture(autouse=True)
def _on_cpu(monkeypatch):
    monkeypatch.setattr(gv, "DEVICE", "cpu")


def _row(golden, e):
    return dict(zip(golden["keys"], golden["routes"][gs.key(e)]))


def exact(golden, wrong=None):
    def launch(e, o):
        row = _row(golden, e)
        if row["rc"] and wrong != "refused":
            return row["rc"], dict(row)
        A = o["A"].view.t() if e["ta"] else o["A"].view
        B = o["B"].view.t() if e["tb"] else o["B"].view
        if wrong == "poison":      # one element from the pitch gap (or the guard) behind A's first row joins the reduction
            A = A.clone()
            A[0, 0] += o["A"].buf[o["A"].off + o["A"].cols]
        w = A.double() @ B.double()
        if o["bias"] is not None:
            b = o["bias"].view[0].double().clone()
            if wrong == "bias":
                b[-1] = 0
            w += b
        if e.get("acc", 0):
            w += o["C"].view.double()
        if e.get("relu", 0):
            w.clamp_(min=0)
        o["C"].view.copy_(w.float())
        sums = A.double().sum(dim=1)
        if wrong == "edge":        # the last row counted twice, as a clamped load would
            sums[-1] *= 2
        for c in o["cs"]:
            c.view[0] += sums.float()
        if wrong == "gap":
            o["C"].buf[o["C"].off + o["C"].cols] = 0.0
        if wrong == "after":
            o["C"].buf[o["C"].off + o["C"].extent] = 0.0
        if wrong == "before":
            o["C"].buf[o["C"].off - 1] = 0.0
        if wrong == "cs_after" and o["cs"]:
            o["cs"][-1].buf[o["cs"][-1].off + e["M"]] = 0.0
        if wrong == "operand":
            o["B"].view[0, 0] += 1.0
        route = dict(row)
        if wrong == "route":
            route["grid"] += 1
        return row["rc"], route
    return launch


def _small(golden):
    return [e for f in gs.FAMILIES for e in gv.family_cases(golden, f) if e["M"] * e["N"] * e["K"] <= 2e7]


def test_exact_launcher_passes_every_small_case(golden):
    cases = _small(golden)
    assert len(cases) > 100 and any(e.get("cs", 0) == 3 for e in cases) and any(e.get("a16", 0) for e in cases)
    n, failed = gv.run_all(cases, exact(golden), golden)
    assert n == len(cases) and not failed, failed


PADDED_C = dict(mode=0, ta=1, tb=0, M=160, N=64, K=96, ldc=68, bias=1)
COLSUMS = dict(mode=0, ta=1, tb=0, M=160, N=64, K=96, lda=164, acc=1, cs=3)


@pytest.mark.parametrize("wrong,e,what", [
    ("gap", PADDED_C, "outside its M x N rectangle"), ("after", PADDED_C, "outside its M x N rectangle"),
    ("before", PADDED_C, "outside its M x N rectangle"), ("bias", PADDED_C, "C: max error"), ("operand", PADDED_C, "B was written"),
    ("route", PADDED_C, "route"), ("edge", COLSUMS, "cs3: max error"), ("cs_after", COLSUMS, "outside its M elements"),
    ("poison", COLSUMS, "NaN in C")])
def test_wrong_launcher_is_reported(wrong, e, what, dump):
    row = gen.routes(dump, [e])[0]
    bad = gv.run_case(e, exact({"keys": list(row), "routes": {gs.key(e): list(row.values())}}, wrong), row)
    assert any(what in b for b in bad), bad


def test_work_for_a_refused_input_is_reported(golden):
    e = next(e for e in gs.table_inputs() if _row(golden, e)["rc"] != 0)
    assert gv.run_case(e, exact(golden), _row(golden, e)) == []
    assert gv.run_case(e, exact(golden, "refused"), _row(golden, e)) == ["a refused product wrote C or the column sums"]


def test_public_entry_is_what_the_exported_entries_can_say():
    p = dict(mode=0, ta=0, tb=1, M=8, N=8, K=8)
    assert gv.public_entry(p) == "xg_gemm" and gv.public_entry(dict(p, lda=12, aA=4, bias=1, relu=1)) == "xg_gemm"
    assert gv.public_entry(dict(p, mode=3, wide=1)) == "xg_gemm_mode" and gv.public_entry(dict(p, mode=1, wide=1)) == "xg_gemm_mode"
    assert gv.public_entry(dict(p, mode=1, wide=1, a16=1, b16=1)) == "xg_gemm_bf16_operands"
    for kw in (dict(bg=1), dict(alone=1), dict(cs=1), dict(no_w1=1), dict(pk_min=2), dict(mode=1), dict(mode=1, wide=1, a16=1),
               dict(mode=3, wide=1, a16=1, b16=1)):
        assert gv.public_entry(dict(p, **kw)) is None, kw
