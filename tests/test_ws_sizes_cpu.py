"""CPU check that no workspace changed size: the recorded table tests/golden/ws_sizes.json (tools/gen_ws_sizes_golden.py, taken
before the step scratch and the searches' shared workspace head were carved by one function each) against the built library.
Blocks may move inside a workspace; callers that cached one of the recorded size must still fit.  No GPU."""
import json
import os
import sys

import pytest

from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def test_workspace_sizes_equal_recorded_table_cpu(built):
    from tools import gen_ws_sizes_golden as gen
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "ws_sizes.json")))
    got = gen.table()
    assert sorted(got) == sorted(want) and len(want) == 2 * len(gen.CONFIGS)
    for key in sorted(want):
        # (a recorded 0 is a refusal: a search needs T >= 2, and W <= V -- `one` has V = 5)
        assert all(v > 0 for v in want[key]["mode"]) and (key.endswith("/T=1") or all(v > 0 for v in want[key]["xgcc"]))
        assert got[key] == want[key], key
