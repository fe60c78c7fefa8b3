"""Run the GEMM sweep of tests/gemm_shapes.py (GEMM_BENCH through xg_gemm_mode in modes 0 / 3 / 1, BF16_OPERANDS in the four layouts
through xg_gemm_bf16_operands) on the product library, one product per case, fixed seeds:

    python tools/gemm_route_sweep.py run [reps [name]]     (cases whose name contains `name`) one JSON line per case: per repetition the sha1 of C and its max error vs float64
    python tools/gemm_route_sweep.py check <kernel_trace.csv>   the GEMM kernels of a rocprofv3 --kernel-trace of `run 1`, in launch
                                                           order, against the planner's routes (tools/gemm_route_dump.cc)

`check` is how a routing change is shown to launch what the planner says: kernel template and workgroups x threads.  (The trace's
LDS column holds a kernel's static bytes only -- 0 for these kernels, whose LDS is all dynamic -- so the route's LDS bytes are printed
beside it, not compared; tests/golden/gemm_routes.json pins them.)"""
import csv
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gemm_shapes as gs  # noqa: E402


def cases():
    """[(name, planner input)] in run order"""
    out = [("%s mode %d" % (name, m), dict(mode=m, wide=int(m != 0), ta=ta, tb=tb, M=M, N=N, K=K, acc=acc))
           for m in (0, 3, 1) for name, ta, tb, M, N, K, acc in gs.GEMM_BENCH]
    out += [("operands %dx%dx%d %d%d" % (M, N, K, ta, tb), dict(mode=1, wide=1, a16=1, b16=1, ta=ta, tb=tb, M=M, N=N, K=K, bias=1))
            for M, N, K in gs.BF16_OPERANDS for ta, tb in gs.LAYOUT_CASES]
    return out


def run(reps, only=""):
    import torch
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    for i, (name, e) in enumerate(cases()):
        if only not in name:
            continue
        M, N, K, ta, tb = e["M"], e["N"], e["K"], e["ta"], e["tb"]
        g = torch.Generator(device="cuda").manual_seed(4000 + i)
        A = torch.randn((K, M) if ta else (M, K), generator=g, device="cuda")
        B = torch.randn((N, K) if tb else (K, N), generator=g, device="cuda")
        bias = torch.randn(N, generator=g, device="cuda")
        C0 = torch.randn(M, N, generator=g, device="cuda")
        if e.get("a16"):
            A16, B16 = A.bfloat16(), B.bfloat16()
            A, B = A16.float(), B16.float()
        sl = slice(0, min(256, M))
        ref = (A.t() if ta else A)[sl].double() @ (B.t() if tb else B).double()
        ref = ref + (bias.double() if e.get("bias") else 0) + (C0[sl].double() if e.get("acc") else 0)
        hashes, errs = [], []
        for _ in range(reps):
            C = C0.clone()
            if e.get("a16"):
                rc = L.xg_gemm_bf16_operands(None, ta, tb, M, N, K, nv.ptr(A), nv.ptr(A16), A.shape[1], nv.ptr(B), nv.ptr(B16), B.shape[1],
                                             nv.ptr(C), N, nv.ptr(bias), 0, 0)
            else:
                rc = L.xg_gemm_mode(None, e["mode"], ta, tb, M, N, K, nv.ptr(A), A.shape[1], nv.ptr(B), B.shape[1], nv.ptr(C), N, None, 0, e["acc"])
            assert rc == 0, (name, rc)
            hashes.append(hashlib.sha1(C.cpu().numpy().tobytes()).hexdigest()[:16])
            errs.append(float("%.3g" % float((C[sl].double() - ref).abs().max() / ref.abs().max())))
        print(json.dumps({"case": name, "hash": hashes, "err": errs}), flush=True)


def kernel_of(e, r):
    """the kernel template instance a route launches, as rocprofv3 prints it"""
    b = lambda x: "true" if x else "false"  # noqa: E731
    akc, bkc, f = b(not e["ta"]), b(e["tb"]), r["family"]
    if f == "gemm_kernel":
        return "gemm_kernel<%d, %d, %s, %s, %s>" % (r["bm"], r["bn"], akc, bkc, b(r["vec"]))
    if f == "gemm_w1":
        return "gemm_w1_kernel<%d, %d, %d, %s, %s>" % (r["bm"], r["bn"], r["bk"], akc, bkc)
    if f == "gemm_pk":
        return "gemm_pk_kernel<128, 128, %s, %s>" % (akc, bkc)
    if f == "gemm_td":
        return "gemm_td_kernel<%d>" % r["ring"]
    if f in ("gemm_bs1", "gemm_bs3"):
        return "gemm_bs_kernel<%s, %s, %s, %s, %s, %s>" % (f[-1], akc, bkc, b(r["vec"]), b(r["a16"]), b(r["b16"]))
    if f == "gemm_bx":
        return "gemm_bx_kernel<256, 128, 4, 2, true, %s>" % bkc
    return "gemm_g16_kernel<%s, %s, %d, %d, %d>" % (akc, bkc, r["bk"], r["ring"], r["threads"] // 256)


def check(trace):
    from tools import gen_gemm_routes_golden as gen
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        routes = gen.routes(gen.build_dump(d), [e for _, e in cs])
    rows = [r for r in csv.DictReader(open(trace)) if "gemm_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    got = [(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0],
            int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"]), int(r["LDS_Block_Size"])) for r in rows]
    assert len(got) == len(cs), (len(got), len(cs))
    bad = 0
    for (name, e), r, g in zip(cs, routes, got):
        want = (kernel_of(e, r), r["grid"], r["threads"])
        ok = want == g[:3]
        bad += not ok
        print("%s %-42s %-52s %6d x %4d  static lds %5d (route: %6d dynamic)" % ("ok " if ok else "BAD", name, g[0], g[1], g[2], g[3], r["lds"]))
    print("cases %d bad %d" % (len(cs), bad))
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 2, sys.argv[3] if len(sys.argv) > 3 else "")
    else:
        sys.exit(1 if check(sys.argv[2]) else 0)
