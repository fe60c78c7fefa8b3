"""The background form of the persistent fp32 GEMM (xg_gemm.hip: gemm_pk_kernel with XGK_GEMM_BG, one workgroup per CU) on products of
a few decoder steps' rows: its unit floor is one 4-slab share for each of the 256 workgroups (tiles x slabs >= 1024), so a product
may consist of stream-K tail only (fewer than 256 tiles: no whole-tile round), of one round plus a tail, or fall under the floor
and take the tile kernels.  Every element against float64."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()

# (the shapes, M x N x K around the floor: tests/gemm_shapes.BG_SMALL_M)
_SCRIPT = r"""
import sys, torch
sys.path.insert(0, %r)
from controllable_xgating_amd import _native as nv
from tests.gemm_shapes import BG_SMALL_M
L = nv.lib()
bad, n = [], 0
def run(M, N, K, acc, it):
    g = torch.Generator(device="cuda").manual_seed(7000 + it)
    A = torch.randn(M, K, generator=g, device="cuda")
    B = torch.randn(N, K, generator=g, device="cuda")
    b = torch.randn(N, generator=g, device="cuda")
    C0 = torch.randn(M, N, generator=g, device="cuda")
    C = C0.clone()
    rc = L.xg_gemm(None, 0, 1, M, N, K, nv.ptr(A), K, nv.ptr(B), K, nv.ptr(C), N, nv.ptr(b), 0, acc)
    want = A.double() @ B.double().t() + b.double() + (C0.double() if acc else 0)
    err = float((C.double() - want).abs().max()) / float(want.abs().max())
    if rc != 0 or not err < 6e-6:
        bad.append((M, N, K, acc, rc, err))
for M, N, K, acc in BG_SMALL_M:
    run(M, N, K, acc, n); n += 1
print("shapes", n, "BAD", bad)
sys.exit(1 if bad else 0)
"""


def test_background_persistent_gemm_small_m_vs_float64():
    """NT layout with bias through xg_gemm with every product forced into the background form (XG_GEMM_FORCE_BG of the -DXG_DIAG
    library; XG_GEMM_NO_W1 keeps the one-round kernel, which refuses real background products, from taking the shapes first).
    Tolerance: the existing fuzz's fp32 bound (test_gemm_fuzz_all_kernels), max error / max |C| < 6e-6."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from controllable_xgating_amd import _native as nv
    env = dict(os.environ, XG_LIBRARY=nv.LIB_DIAG_PATH, XG_GEMM_FORCE_BG="1", XG_GEMM_NO_W1="1")
    env.pop("XG_PK_MIN", None)             # the production floor is what is under test
    r = subprocess.run([sys.executable, "-c", _SCRIPT % root], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
