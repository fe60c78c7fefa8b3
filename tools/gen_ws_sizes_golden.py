"""Record the workspace sizes the library reports (host only, no GPU) into tests/golden/ws_sizes.json:

    [XG_LIBRARY=<another build>] python tools/gen_ws_sizes_golden.py [--check]

xg_workspace_bytes_mode (modes 0, 1, 3), xgcb_workspace_bytes (W), xgcc_workspace_bytes (S) and xgbc_workspace_bytes (S, W) over the
tests/util.py configurations below at T = 1 and T = L + 1.  tests/test_ws_sizes_cpu.py asserts the table against the built
library: a change of a carve function may move blocks inside a workspace, not resize one.  --check compares instead of writing."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "ws_sizes.json")
CONFIGS = ("tiny", "odd", "one", "mid", "c1", "c5")
MODES, WS, SS = (0, 1, 3), (1, 3, 5, 8), (1, 2, 5, 8)


def table():
    """{"<config>/T=<T>": {"mode": [..], "xgcb": [..], "xgcc": [..], "xgbc": [[W ..] per S]}} from the loaded library."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_beam as nb
    from controllable_xgating_amd import _native_beam_control as nbc
    from controllable_xgating_amd import _native_control as ncc
    from tests import util
    out = {}
    for name in CONFIGS:
        c = util.CFG[name]
        for T in (1, c["L"] + 1):
            d = nv.XgDims(c["B"], c["K"], c["R"], c["A"], c["E"], c["V"], c["C"], c["H"], c["F1"], c["F2"], T)
            p = C.byref(d)
            out["%s/T=%d" % (name, T)] = {
                "mode": [int(nv.lib().xg_workspace_bytes_mode(p, m)) for m in MODES],
                "xgcb": [int(nb.lib().xgcb_workspace_bytes(p, W)) for W in WS],
                "xgcc": [int(ncc.lib().xgcc_workspace_bytes(p, S)) for S in SS],
                "xgbc": [[int(nbc.lib().xgbc_workspace_bytes(p, S, W)) for W in WS] for S in SS]}
    return out


if __name__ == "__main__":
    t = table()
    if "--check" in sys.argv[1:]:
        want = json.load(open(PATH))
        bad = [k for k in want if want[k] != t.get(k)]
        print("equal" if not bad and len(want) == len(t) else "DIFFERENT: %s" % bad)
        sys.exit(1 if bad or len(want) != len(t) else 0)
    with open(PATH, "w") as f:
        json.dump(t, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", PATH, len(t), "entries")
