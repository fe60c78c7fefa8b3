"""Test helper of tests/test_gpu_gemm_variants.py: one planner input of tests/gemm_shapes.py launched as a bare product inside
poisoned allocations and checked against float64.

    python -m tests.gemm_variant_run <family>       (with XG_LIBRARY = the -DXG_DIAG library)

runs every variant of the family (gemm_shapes.variant_cases) through xg_debug_gemm_planned (csrc/xg_gemm.hip), which plans with the
tuning of the call and reports the route it launched.  The key of a case is printed before its launch; the process ends at the first
return code or HIP error and starts nothing after it.  run_case() is also what the parent test hands the product library's public
entries.

Operands.  A, B (their bf16 mirrors), C, the bias and the column-sum accumulators each live in an allocation of their own: GUARD
quiet-NaN elements, the data at the input's address % 16 and pitch, GUARD more.  The pitch gaps are quiet NaN too.  Values are
seeded randn; where an operand has a mirror the fp32 operand holds the mirror's values exactly.

Bounds (the tests that own them: test_gemm_layouts, test_gemm_bf16_operands_in_memory, test_gemm_bf16_modes):
  fp32 kernels, and plain bf16 whose operands ARE bf16 values (both mirrors)     (2e-6 sqrt(K) 4 + 1e-6) max(1, max |want|)
  split-bf16                                                                     4e-6 max |want|
  plain bf16 that rounds an fp32 operand                                         2e-2 max |want|
Column sums: the product's own bound with N = 1, and never looser than the first: split-bf16 keeps its 4e-6, plain bf16 takes the
first.  That holds in mode 1 without a mirror of A as well: tests/bf16_oracle.py ("db") sums the fp32 values there, and so does the
kernel (gemm_bs_kernel: cs_add adds the registers it loaded, before they are rounded); with a mirror the mirror is summed, and the
fp32 operand here holds exactly those values."""
import ctypes as C
import json
import math
import sys
import time

import torch

from tests import gemm_shapes as gs

GUARD = 4096           # quiet-NaN elements before and after every allocation's data
DEVICE = "cuda"        # (tests/test_gemm_variant_run_cpu.py checks the checks themselves on "cpu")
WIDE = ("gemm_bs1", "gemm_bs3", "gemm_bx", "g16")
TUNE_KEYS = ("no_pk", "pk_min", "no_bg", "force_bg", "no_w1", "w1_bm", "w1_bn", "force_tile", "force_splitk", "x3_fp32", "no_td", "td_all",
             "td_ks", "td_depth", "no_bx", "no_g16", "g16_cfg")                       # tools/gemm_route_dump.cc
TUNE_DEFAULTS = dict(pk_min=-1, force_splitk=1, x3_fp32=1, td_depth=8, g16_cfg=-1)  # csrc/xg_gemm_route.h: XgGemmTuning
ROUTE_OUT = ("rc", "family", "planes", "bm", "bn", "bk", "vec", "fast", "a16", "b16", "splitk", "grid", "threads", "gm", "rounds", "tail_wgs",
             "ring", "cfg", "lds", "pad_lds", "clear", "r0", "c0", "rows", "cols", "colsum")
FAMILY_NAMES = {0: "none", 1: "gemm_kernel", 2: "gemm_w1", 3: "gemm_pk", 4: "gemm_td", 5: "gemm_bs", 6: "gemm_bx", 7: "g16"}      # XgGemmFamily
CLEAR_RECT = 2


def golden_table():
    from tools import gen_gemm_routes_golden as gen
    with open(gen.PATH) as f:
        return json.load(f)


def family_cases(golden, family):
    """the inputs of gemm_shapes.variant_cases whose route is of `family`, in table order; the refused input (no family) runs with
    the first one"""
    return [e for v, e in gs.variant_cases(golden).items() if v[1] == family or (v[1] == "none" and family == gs.FAMILIES[0])]


def public_entry(e):
    """the exported entry that hands the planner exactly this input, or None: no tuning, no bg / alone / column sums, both mirrors
    or neither"""
    if any(e.get(k, 0) for k in TUNE_KEYS + ("bg", "alone", "cs")) or bool(e.get("a16", 0)) != bool(e.get("b16", 0)):
        return None
    if e["mode"] == 0:      # (xg_gemm plans with wide_forced false and no mirrors)
        return None if e.get("a16", 0) or e.get("wide", 0) else "xg_gemm"
    if not e.get("wide", 0):
        return None
    if e.get("a16", 0):
        return "xg_gemm_bf16_operands" if e["mode"] == 1 else None
    return "xg_gemm_mode"


class Block:
    """rows x cols elements at pitch ld whose first one sits `align` bytes past a 16-byte boundary, in the middle of a quiet-NaN
    allocation.  (A pitch shorter than the row -- the table has lda = 1001 under 2688-element rows -- makes rows overlap: legal for
    an operand that is only read, and then there is no gap to poison.)"""

    def __init__(self, rows, cols, ld, align, dtype, gen=None, values=None):
        es = torch.empty((), dtype=dtype).element_size()
        assert align % es == 0 and 0 <= align < 16 and rows > 0 and cols > 0
        self.rows, self.cols, self.ld = rows, cols, ld
        self.extent = (rows - 1) * ld + cols
        self.off = GUARD + align // es
        self.buf = torch.full((self.off + self.extent + GUARD,), float("nan"), dtype=dtype, device=DEVICE)
        assert self.buf.data_ptr() % 16 == 0
        flat = self.buf[self.off:self.off + self.extent]
        flat.copy_(values if values is not None else torch.randn(self.extent, generator=gen, device=DEVICE))
        if ld > cols and rows > 1:
            torch.as_strided(self.buf, (rows - 1, ld - cols), (ld, 1), self.off + cols).fill_(float("nan"))
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.off)
        self.address = self.buf.data_ptr() + self.off * es
        assert self.address % 16 == align
        self.before = self.buf.clone()

    @property
    def flat(self):
        return self.buf[self.off:self.off + self.extent]

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    def _bits(self, t):
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16)

    def unchanged(self):
        return torch.equal(self._bits(self.buf), self._bits(self.before))

    def unchanged_outside(self):
        """bit-identical to before the call everywhere but the rows x cols rectangle"""
        now = self.buf.clone()
        torch.as_strided(now, (self.rows, self.cols), (self.ld, 1), self.off).copy_(
            torch.as_strided(self.before, (self.rows, self.cols), (self.ld, 1), self.off))
        return torch.equal(self._bits(now), self._bits(self.before))

    def start(self):
        """the rectangle as it was before the call"""
        return torch.as_strided(self.before, (self.rows, self.cols), (self.ld, 1), self.off)


def _sync():
    if DEVICE == "cuda":
        torch.cuda.synchronize()


def _none():
    return C.c_void_p(None)


def make_operands(e):
    ta, tb, M, N, K = e["ta"], e["tb"], e["M"], e["N"], e["K"]
    la, lb, lc = gs.row_lengths(e)
    lda, ldb, ldc = e.get("lda", 0) or la, e.get("ldb", 0) or lb, e.get("ldc", 0) or lc
    assert ldc >= N
    gen = torch.Generator(device=DEVICE).manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(gs.key(e))) % (1 << 31))
    o = dict(lda=lda, ldb=ldb, ldc=ldc)
    for name, rows, cols, ld, al, al16 in (("A", K if ta else M, la, lda, e.get("aA", 0), e.get("aA16", 0)),
                                           ("B", N if tb else K, lb, ldb, e.get("aB", 0), e.get("aB16", 0))):
        if e.get(name.lower() + "16", 0):
            o[name + "16"] = Block(rows, cols, ld, al16, torch.bfloat16, gen)
            o[name] = Block(rows, cols, ld, al, torch.float32, values=o[name + "16"].flat.float())
        else:
            o[name + "16"] = None
            o[name] = Block(rows, cols, ld, al, torch.float32, gen)
    o["C"] = Block(M, N, ldc, e.get("aC", 0), torch.float32, gen)
    o["bias"] = Block(1, N, N, 0, torch.float32, gen) if e.get("bias", 0) else None
    o["cs"] = [Block(1, M, M, 0, torch.float32, gen) for _ in range(e.get("cs", 0))]      # seeded randn: non-zero starts
    return o


def reference_errors(e, o):
    """(max |C - want|, max |want|, max |cs - want_cs| per accumulator, max |want_cs|, NaN seen) against float64, in row blocks"""
    ta, tb, M, N, K = e["ta"], e["tb"], e["M"], e["N"], e["K"]
    Bd = (o["B"].view.t() if tb else o["B"].view).double()
    bias = o["bias"].view[0].double() if o["bias"] is not None else None
    C0, Cn = o["C"].start(), o["C"].view
    step = max(1, min(M, (1 << 25) // max(K, N, 1)))
    err = scale = 0.0
    cs_err, cs_scale = [0.0] * len(o["cs"]), 0.0
    nan = False
    for r in range(0, M, step):
        a = (o["A"].view[:, r:r + step].t() if ta else o["A"].view[r:r + step]).double()
        want = a @ Bd
        if bias is not None:
            want += bias
        if e.get("acc", 0):
            want += C0[r:r + step].double()
        if e.get("relu", 0):
            want.clamp_(min=0)
        got = Cn[r:r + step].double()
        nan = nan or bool(torch.isnan(got).any())
        err = max(err, float((got - want).abs().max()))
        scale = max(scale, float(want.abs().max()))
        if o["cs"]:
            sums = a.sum(dim=1)
            for i, c in enumerate(o["cs"]):
                w = c.start()[0, r:r + step].double() + sums
                g = c.view[0, r:r + step].double()
                nan = nan or bool(torch.isnan(g).any())
                cs_err[i] = max(cs_err[i], float((g - w).abs().max()))
                cs_scale = max(cs_scale, float(w.abs().max()))
    return err, scale, cs_err, cs_scale, nan


def bound(e, family):
    """(absolute bound as a function of max |want|, its name)"""
    K = e["K"]
    if family == "gemm_bs3":
        return (lambda s: 4e-6 * s), "split-bf16 4e-6"
    if family in WIDE and not (e.get("a16", 0) and e.get("b16", 0)):
        return (lambda s: 2e-2 * s), "bf16 2e-2"
    return (lambda s: (2e-6 * math.sqrt(K) * 4 + 1e-6) * max(1.0, s)), "fp32"


def run_case(e, launch, row):
    """Launch `e` with launch(e, operands) -> (return code, route values in the table's key order or None) and check it against
    `row`, the recorded route of the input as {key: value}.  Returns the list of what failed (empty: the case passed)."""
    o = make_operands(e)
    _sync()
    rc, route = launch(e, o)
    _sync()                       # (a HIP error raises here: the caller starts nothing after it)
    bad = []
    if rc != row["rc"]:
        return ["return code %d, the table says %d" % (rc, row["rc"])]
    if route is not None and row["rc"] == 0 and route != row:
        bad.append("route %s, the table says %s" % ({k: v for k, v in route.items() if row[k] != v}, {k: v for k, v in row.items() if route[k] != v}))
    for name in ("A", "A16", "B", "B16", "bias"):
        if o[name] is not None and not o[name].unchanged():
            bad.append("%s was written" % name)
    if row["rc"] != 0:      # refused: nothing may have been touched
        if not o["C"].unchanged() or not all(c.unchanged() for c in o["cs"]):
            bad.append("a refused product wrote C or the column sums")
        return bad
    if not o["C"].unchanged_outside():
        bad.append("C was written outside its M x N rectangle")
    if not all(c.unchanged_outside() for c in o["cs"]):
        bad.append("a column-sum accumulator was written outside its M elements")
    err, scale, cs_err, cs_scale, nan = reference_errors(e, o)
    if nan:
        bad.append("NaN in C or the column sums")
    lim, name = bound(e, row["family"])
    print("    err %.3e of %.3e (%s, max |want| %.3e)" % (err, lim(scale), name, scale), flush=True)
    if not err <= lim(scale):
        bad.append("C: max error %.3e over the %s bound %.3e (max |want| %.3e)" % (err, name, lim(scale), scale))
    cs_lim = min(lim(cs_scale), (2e-6 * math.sqrt(e["K"]) * 4 + 1e-6) * max(1.0, cs_scale))
    for i, ce in enumerate(cs_err):
        print("    cs%d err %.3e of %.3e" % (i + 1, ce, cs_lim), flush=True)
        if not ce <= cs_lim:
            bad.append("cs%d: max error %.3e over %.3e (max |want| %.3e)" % (i + 1, ce, cs_lim, cs_scale))
    return bad


# ---- the diag library's entry
def diag_launcher(path, keys):
    L = C.CDLL(path)
    f = L.xg_debug_gemm_planned
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [C.c_void_p] * 9 +[C.POINTER(C.c_int32)]

    def launch(e, o):
        la, lb, lc = o["lda"], o["ldb"], o["ldc"]
        inp = (C.c_int32 * 14)(e["mode"], e.get("wide", 0), e["ta"], e["tb"], e["M"], e["N"], e["K"], la, lb, lc, e.get("relu", 0),
                               e.get("acc", 0), e.get("bg", 0), e.get("alone", 0))
        tune = (C.c_int32 * 19)(*[e.get(k, 0) or TUNE_DEFAULTS.get(k, 0) for k in TUNE_KEYS], int("w1_bm" in e), int("force_tile" in e))
        out = (C.c_int32 * len(ROUTE_OUT))()
        cs = [c.ptr for c in o["cs"]] + [_none()] * (3 - len(o["cs"]))
        rc = f(None, inp, tune, o["A"].ptr, o["A16"].ptr if o["A16"] else _none(), o["B"].ptr, o["B16"].ptr if o["B16"] else _none(),
               o["C"].ptr, o["bias"].ptr if o["bias"] else _none(), cs[0], cs[1], cs[2], out)
        r = dict(zip(ROUTE_OUT, out))
        r["family"] = FAMILY_NAMES[r["family"]] + (str(r["planes"]) if r["family"] == 5 else "")
        r["rect"] = [r["r0"], r["c0"], r["rows"], r["cols"]] if r["clear"] == CLEAR_RECT else []
        return rc, {k: r[k] for k in keys}
    return launch


# ---- the product library's public entries
def public_launch(e, o):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    entry = public_entry(e)
    head = (e["ta"], e["tb"], e["M"], e["N"], e["K"])
    tail = (o["C"].ptr, o["ldc"], o["bias"].ptr if o["bias"] else None, e.get("relu", 0), e.get("acc", 0))
    if entry == "xg_gemm":
        return L.xg_gemm(None, *head, o["A"].ptr, o["lda"], o["B"].ptr, o["ldb"], *tail), None
    if entry == "xg_gemm_mode":
        return L.xg_gemm_mode(None, e["mode"], *head, o["A"].ptr, o["lda"], o["B"].ptr, o["ldb"], *tail), None
    assert entry == "xg_gemm_bf16_operands"
    return L.xg_gemm_bf16_operands(None, *head, o["A"].ptr, o["A16"].ptr, o["lda"], o["B"].ptr, o["B16"].ptr, o["ldb"], *tail), None


def run_all(cases, launch, golden):
    """every case in order; (number run, {key: what failed}).  A HIP error or an unexpected return code ends the run."""
    failed = {}
    for n, e in enumerate(cases):
        k = gs.key(e)
        print("case %d: %s" % (n, k), flush=True)
        row = dict(zip(golden["keys"], golden["routes"][k]))
        bad = run_case(e, launch, row)
        if bad:
            failed[k] = bad
            print("    FAILED: " + "; ".join(bad), flush=True)
            if bad[0].startswith("return code"):
                return n + 1, failed
    return len(cases), failed


def main(family):
    from controllable_xgating_amd import _native as nv
    assert nv.LIB_PATH == nv.LIB_DIAG_PATH, "run with XG_LIBRARY = the diag library"
    golden = golden_table()
    cases = family_cases(golden, family)
    t0 = time.time()
    n, failed = run_all(cases, diag_launcher(nv.LIB_PATH, golden["keys"]), golden)
    print("%s: %d of %d variants run in %.1f s, %d failed" % (family, n, len(cases), time.time() - t0, len(failed)), flush=True)
    for k, bad in failed.items():
        print("FAILED %s: %s" % (k, "; ".join(bad)))
    return 3 if failed or n != len(cases) else 0      # (3: every launch came back and something is wrong; a HIP error raises instead)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
