"""Every kernel variant the GEMM planner can name, launched as a bare product against float64.

tests/golden/gemm_routes.json says which kernel a shape gets; this says that the kernel computes the product when it is launched
that way.  tests/gemm_shapes.variant_cases picks, per variant (what selects a template instance or a code path inside a kernel), the
cheapest input of the table; tests/gemm_variant_run.py runs each one through xg_debug_gemm_planned of the -DXG_DIAG library -- the
planner, the clears, the column-sum pass and the family switch of xgk_gemm_run, with the input's tuning for that call -- inside
allocations whose every element outside the logical rectangles is a quiet NaN.  Per case: the launched route is the recorded one;
C, and each column-sum accumulator, match float64 within the bound of the test that owns the kernel's class (gemm_variant_run's
docstring has the three bounds and the column sums' own); no NaN reaches C or the sums; nothing outside
the M x N rectangle of C, the M elements of an accumulator or the bias changes by a bit; the operands are unchanged.  The one input
the planner refuses must return its code and touch nothing.

One child process per family (a fault ends that child and nothing is launched after it: the remaining families then fail without
starting anything on the card); the inputs the three public entries can express then run again here through the product library,
same buffers, same assertions but the route."""
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_shapes as gs
from tests import gemm_variant_run as gv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STOPPED = []      # why nothing more is started: a child that did not end by itself (exit 0, or 3: numerical failures only), a HIP error here


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(scope="module")
def golden():
    return gv.golden_table()


@pytest.mark.parametrize("family", gs.FAMILIES)
def test_family_variants_match_float64_inside_poison(family, golden):
    from controllable_xgating_amd import _native as nv
    assert not _STOPPED, "not started: " + _STOPPED[0]
    cases = gv.family_cases(golden, family)
    assert cases, "no variant of " + family
    env = dict(os.environ, XG_LIBRARY=nv.LIB_DIAG_PATH)
    for k in list(env):      # the tuning is per call: no process-wide switch may be set
        if k.startswith(("XG_GEMM_", "XG_PK_", "XG_TD_", "XG_W1_", "XG_G16_", "XG_NO_", "XG_X3_")):
            del env[k]
    try:
        r = subprocess.run([sys.executable, "-m", "tests.gemm_variant_run", family], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        _STOPPED.append("the child of %s did not finish" % family)
        raise
    if r.returncode not in (0, 3):
        _STOPPED.append("the child of %s ended with exit %d" % (family, r.returncode))
    print("\n".join(r.stdout.splitlines()[-3:]))
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, "\n".join(r.stdout.splitlines()[-30:]), r.stderr[-3000:])
    # the product build is what ships: its kernels are compiled without XG_DIAG
    assert not hasattr(nv.lib(), "xg_debug_gemm_planned")
    public = [e for e in cases if gv.public_entry(e)]
    try:
        n, failed = gv.run_all(public, gv.public_launch, golden)
    except Exception as ex:      # (a HIP error at the synchronize after a launch)
        _STOPPED.append("the product-library pass of %s raised %r" % (family, ex))
        raise
    print("%s: %d of %d variants again through the product library" % (family, n, len(cases)))
    assert not failed and n == len(public), failed
