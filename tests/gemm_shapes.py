"""The GEMM shape lists of the GPU tests and of tools/ubench/gemm_bench.py in one place, and the table of planner inputs
(csrc/xg_gemm_route.h: xg_gemm_plan) that tools/gen_gemm_routes_golden.py records and tests/test_gemm_routes_cpu.py pins.

A planner input is a dict of the keys tools/gemm_route_dump.cc reads (anything absent is 0 / the tuning default).  `cs` counts the
column-sum accumulators (1 to 3): the planner only sees that there are some, tests/test_gpu_gemm_variants.py passes that many."""
LAYOUT_CASES = [(0, 1), (0, 0), (1, 0), (1, 1)]                      # (ta, tb): NT forward, NN data gradient, TN weight gradient, TT
EPILOGUES = ((0, 0), (1, 0), (0, 1))                                 # (relu, accumulate) every GEMM test runs

# tests/test_gpu_parity.py
LAYOUTS = [(128, 2048, 1536), (2688, 512, 468), (37, 53, 29), (8, 1536, 1024), (300, 260, 131), (64, 64, 32), (1, 5, 7), (513, 129, 1000)]
PERSISTENT = [(2688, 2000, 516), (1300, 9000, 200), (1408, 512, 20000), (3000, 3000, 256), (2688, 20000, 512), (4100, 2052, 96)]
BF16_OPERANDS = [(256, 256, 128), (2688, 1000, 1024), (328, 2048, 2688), (1408, 512, 20000), (136, 264, 200), (5120, 1024, 1536)]
BF16_MODES = [(512, 384, 300), (300, 200, 129), (2688, 512, 468)]
W1_SHAPES = ((1000, 516, 512), (3328, 512, 1536), (260, 2052, 256))          # test_gemm_one_workgroup_per_cu_kernel
W1_TILE_CASES = ["auto", "64,64", "64,128", "128,64", "128,128", "128,192", "192,128", "128,256", "256,128"]
TD_SHAPES = ((2048, 512, 2688), (20000, 512, 2688), (512, 512, 3328), (516, 468, 1040), (1536, 512, 2688), (2048, 468, 2688),
             (512, 1024, 3328), (4100, 260, 272))                            # test_gemm_weight_gradient_layout_from_memory
TD_RULES = {"production": {}, "every_eligible_product": dict(td_all=1), "split_2": dict(td_all=1, td_ks=2), "depth_4": dict(td_all=1, td_depth=4)}

# tests/test_gpu_bg_small_m.py: (M, N, K, accumulate) in run order, NT with bias.  Tiles are 128 x 128 and slabs 32 deep: K = 64 /
# 468 / 512 are 2 / 15 (the last one partial) / 16 slabs.  640 x 2504 x 512 is 100 tiles = 1600 units: above the floor with every
# tile in the tail; 384 x 2504 x 512 is 960 units: just under it; 128 x 128 is one tile.  M = 200 and 392, N = 1000 and 2504 leave
# ragged edge tiles.
BG_SMALL_M = [(M, N, K, 0) for M in (128, 200, 256, 384, 392, 640) for N in (128, 1000, 2504) for K in (64, 468, 512)] + [
    (640, 2504, 512, 1),       # += C on the all-tail shape: every share adds with atomics, nothing is zeroed
    (392, 2504, 468, 1),
    (384, 20000, 512, 0),      # three decoder steps of the flagship shape: 471 tiles = one round + a 215-tile tail
    (256, 20000, 512, 0)]      # two steps: 314 tiles = one round + 58

# tools/ubench/gemm_bench.py: name, ta, tb, M, N, K, acc
GEMM_BENCH = [
    ("logits fwd NT", 0, 1, 2688, 20000, 512, 0),
    ("dW_logit TN", 1, 0, 20000, 512, 2688, 1),
    ("dH NN K=20000", 0, 0, 2688, 512, 20000, 0),
    ("wgrad TN 2048x512 K=2688", 1, 0, 2048, 512, 2688, 1),
    ("enc embed NT 3328x512 K=1536", 0, 1, 3328, 512, 1536, 0),
    ("PRE NT 3328x2048 K=512", 0, 1, 3328, 2048, 512, 0),
    ("vproj NT 3328x1536 K=512", 0, 1, 3328, 1536, 512, 0),
    ("dX NN 3328x512 K=2048", 0, 0, 3328, 512, 2048, 0),
    ("rollout logits NT 128x20000 K=512", 0, 1, 128, 20000, 512, 0),
    ("rollout logits NT 64x20000 K=512", 0, 1, 64, 20000, 512, 0),
    ("dH NN 1920x512 K=20000", 0, 0, 1920, 512, 20000, 0),
    ("dH half NN 1408x512 K=20000", 0, 0, 1408, 512, 20000, 0),
    ("dH half NN 1280x512 K=20000", 0, 0, 1280, 512, 20000, 0),
    # the teacher-forced forward's vocabulary product in step-sized chunks (with XG_GEMM_FORCE_BG=1: the background form they run in)
    ("logits chunk NT 256x20000 K=512", 0, 1, 256, 20000, 512, 0),
    ("logits chunk NT 384x20000 K=512", 0, 1, 384, 20000, 512, 0),
    ("logits chunk NT 512x20000 K=512", 0, 1, 512, 20000, 512, 0),
    ("logits chunk NT 1280x20000 K=512", 0, 1, 1280, 20000, 512, 0),
]

FAMILIES = ("gemm_kernel", "gemm_w1", "gemm_pk", "gemm_td", "gemm_bs1", "gemm_bs3", "gemm_bx", "g16")
POLICY_CONFIGS = ("tiny", "mid", "c1", "c5")                         # c5: the hidden-1024 configuration
NO_PERSISTENT = dict(no_td=1, no_w1=1, no_pk=1)                      # what is left is gemm_kernel's own tile / split rule


def key(e):
    """the input line of tools/gemm_route_dump.cc (zeros, which are its defaults, left out)"""
    return " ".join("%s=%d" % (k, v) for k, v in e.items() if v != 0)


def _p(M, N, K, ta, tb, mode=0, **kw):
    e = dict(mode=mode, ta=ta, tb=tb, M=M, N=N, K=K)
    e.update(kw)
    return e


def gpu_test_inputs():
    """what the existing GPU GEMM tests and tools/ubench/gemm_bench.py hand the planner (default tuning unless the test sets a
    switch): {source: [inputs]}"""
    out = {}
    out["test_gemm_layouts"] = [_p(M, N, K, ta, tb, bias=1, relu=r, acc=a) for M, N, K in LAYOUTS for ta, tb in LAYOUT_CASES for r, a in EPILOGUES]
    out["test_gemm_persistent_kernel_shapes"] = [_p(M, N, K, ta, tb, bias=1, relu=r, acc=a)
                                                 for M, N, K in PERSISTENT for ta, tb in LAYOUT_CASES for r, a in EPILOGUES]
    out["test_gemm_bf16_operands_in_memory"] = [_p(M, N, K, ta, tb, mode=1, wide=1, a16=1, b16=1, bias=1, relu=r, acc=a)
                                                for M, N, K in BF16_OPERANDS for ta, tb in LAYOUT_CASES for r, a in EPILOGUES]
    out["test_gemm_bf16_modes"] = [_p(M, N, K, ta, tb, mode=m, wide=1, bias=1, relu=r, acc=a)
                                   for M, N, K in BF16_MODES for ta, tb in LAYOUT_CASES for m in (3, 1) for r, a in EPILOGUES]
    out["test_gpu_bg_small_m"] = [_p(M, N, K, 0, 1, bias=1, acc=a, force_bg=1, no_w1=1) for M, N, K, a in BG_SMALL_M]
    w1 = [{} if t == "auto" else dict(zip(("w1_bm", "w1_bn"), map(int, t.split(",")))) for t in W1_TILE_CASES]
    out["test_gemm_one_workgroup_per_cu_kernel"] = [_p(M, N, K, ta, tb, bias=1, relu=r, acc=a, **t)
                                                    for t in w1 for M, N, K in W1_SHAPES for ta, tb in LAYOUT_CASES for r, a in EPILOGUES
                                                    if not t or (r, a) == (0, 0)]      # (forced tiles: the route does not depend on the epilogue)
    out["test_gemm_weight_gradient_layout_from_memory"] = [_p(M, N, K, 1, 0, acc=a, **t) for t in TD_RULES.values() for M, N, K in TD_SHAPES for a in (0, 1)]
    out["gemm_bench"] = [_p(M, N, K, ta, tb, mode=m, wide=int(m != 0), acc=a) for _, ta, tb, M, N, K, a in GEMM_BENCH for m in (0, 3, 1)]
    return out


def policy_inputs():
    """every product tests/bf16_oracle.policy_table lists for the teacher-forced iteration of POLICY_CONFIGS, in modes 0 / 1 / 3, as
    xg_model.hip issues it: forward NT with bias, data gradient NN, weight gradient TN accumulating, with the column sums where the
    bias gradient rides in it; bf16 mirrors of both operands in mode 1.  XGK_GEMM_ALONE: the encoder's weight gradients behind the
    recurrence (embedding, weight_ih, weight_hh).  XGK_GEMM_BG: the vocabulary head's weight gradient and (a second entry) its data
    gradient beside the reverse-time loop, which all four configurations overlap (K <= 48 frames), and in mode 0 the vocabulary
    forward beside the decoder loop."""
    from oracle import paramgen as pg
    from tests import bf16_oracle as bo
    from tests.util import CFG
    out = []
    for name in POLICY_CONFIGS:
        tab = bo.policy_table(pg.make_dims(**CFG[name]), "xe")
        for (site, kind), (M, N, K, _, _) in sorted(tab.items()):
            if kind not in ("fwd", "dx", "dw") or M <= 0 or K <= 0:
                continue
            for mode in (0, 1, 3):
                mir = dict(a16=1, b16=1) if mode == 1 else {}
                enc_dw = kind == "dw" and site.startswith(bo.ENC) and ("visual_emb" in site or "lstmcell" in site)
                if kind == "fwd":
                    out.append(_p(M, N, K, 0, 1, mode, bias=1, bg=int(site == "logit" and mode == 0), **mir))
                elif kind == "dx":
                    out.append(_p(M, N, K, 0, 0, mode, **mir))
                    if site == "logit":
                        out.append(_p(M, N, K, 0, 0, mode, bg=1, **mir))
                else:
                    rides = tab[(site, "db")][0] > 0
                    out.append(_p(M, N, K, 1, 0, mode, acc=1, cs=int(rides), alone=int(enc_dw), bg=int(site == "logit"), **mir))
    return out


def threshold_inputs():
    """the two shapes on either side of every threshold of the planner, unaligned operands, ReLU on and off"""
    out = []

    def both(M, N, K, ta, tb, mode=0, **kw):
        for relu in (0, 1):
            out.append(_p(M, N, K, ta, tb, mode, relu=relu, **kw))

    # gemm_kernel: t128 383 / 384 and 1023 / 1024 (nslab 4 and 32: split in two from 32 slabs), few tiles under a deep reduction
    # (t128 31 / 32, nslab 255 / 256), t64 3 / 4 -- with and without the persistent kernels in front
    for tune in ({}, NO_PERSISTENT):
        for nt in (383, 384, 1023, 1024):
            for K in (128, 1024):
                both(128, 128 * nt, K, 0, 1, **tune)
        for M, N in ((128, 128 * 31), (512, 1024)):
            for K in (8160, 8192):
                both(M, N, K, 0, 0, **tune)
        for M, N in ((64, 192), (128, 128), (128, 64)):
            both(M, N, 2048, 0, 1, **tune); both(M, N, 2048, 1, 0, **tune)
    # the bf16 family's floor (modes 1 and 3; mode 3 keeps the weight-gradient layout in fp32)
    for mode in (1, 3):
        for M, N, K in ((255, 64, 256), (256, 64, 256), (256, 63, 256), (256, 64, 255), (256, 64, 252), (4096, 4096, 4096)):
            for ta, tb in LAYOUT_CASES:
                both(M, N, K, ta, tb, mode)
    # fast loads: byte offsets below 2^31, at least 4 rows
    for M in (524287, 524288):
        both(M, 64, 1024, 0, 1)
    for M in (3, 4):
        both(M, 512, 512, 0, 1); both(512, M, 512, 0, 1)
    # gemm_td: M / N 60 / 64, K 240 / 256, tiles 31 / 32 (alone), 191 / 192 (split), 1023 / 1024 (no flag), background LDS padding
    for M, N, K in ((60, 2048, 512), (64, 2048, 512), (2048, 60, 512), (2048, 64, 240), (2048, 64, 256), (64 * 31, 64, 512),
                    (64 * 191, 64, 4096), (64 * 192, 64, 4096), (64 * 1023, 64, 512), (64 * 1024, 64, 512), (2048, 512, 2688)):
        for flags in ({}, dict(alone=1), dict(bg=1)):
            out.append(_p(M, N, K, 1, 0, acc=1, cs=1, **flags))
            out.append(_p(M, N, K, 1, 0, **flags))
    out.append(_p(2048, 512, 2688, 1, 0, alone=1, bias=1)); out.append(_p(2048, 512, 2688, 1, 0, alone=1, relu=1))
    out.append(_p(2048, 512, 2688, 1, 0, alone=1, aC=4)); out.append(_p(2048, 512, 2688, 1, 0, alone=1, ldc=514))
    for depth in (4, 12):
        out.append(_p(2048, 512, 2688, 1, 0, alone=1, td_depth=depth)); out.append(_p(64 * 31 + 64, 64, 256, 1, 0, alone=1, td_depth=depth))
    # gemm_w1: K 224 / 256, the 0.70 coverage floor, more than 256 tiles of the largest candidate, column sums, background
    for M, N, K in ((1024, 1024, 224), (1024, 1024, 256), (1024, 1024, 512), (1100, 1000, 512), (700, 600, 512), (2048, 2048, 256),
                    (2049, 2048, 256), (4096, 2048, 256), (4097, 2048, 256), (96, 96, 512), (300, 260, 512)):
        both(M, N, K, 0, 1)
        for ta, tb in LAYOUT_CASES[1:]:
            out.append(_p(M, N, K, ta, tb))
    out.append(_p(1024, 1024, 512, 0, 1, bg=1)); out.append(_p(1024, 1024, 512, 1, 0, cs=1))
    for bm, bn in ((64, 64), (64, 128), (128, 64), (128, 128), (128, 192), (192, 128), (128, 256), (256, 128)):
        out.append(_p(1024, 1024, 512, 0, 1, w1_bm=bm, w1_bn=bn))
    # gemm_pk: the 512 x 40 unit floor (512 tiles of 39 / 40 slabs), ReLU with 511 / 512 tiles, a tail rectangle that cannot be
    # cleared (C unaligned, ldc % 4), background floor and padding
    for K in (1248, 1280):
        both(2048, 4096, K, 0, 1, no_w1=1)
    for N in (128 * 511, 128 * 512, 128 * 513):
        both(128, N, 4096, 0, 1, no_w1=1)
    for kw in (dict(), dict(aC=4), dict(ldc=2001), dict(acc=1), dict(bg=1), dict(bg=1, no_bg=1), dict(pk_min=2), dict(no_pk=1)):
        out.append(_p(2688, 2000, 516, 0, 1, **kw))
    # the register-staged bf16 kernels: 511 / 512 tiles (split), the 256 x 128 kernel from M = 256 and under 255 / 256 of its tiles
    for mode in (1, 3):
        for M, N, K in ((128 * 511, 128, 1024), (128 * 512, 128, 1024), (255, 4096, 1024), (256, 4096, 1024), (256 * 15, 128 * 17, 2048),
                        (256 * 16, 128 * 16, 2048), (2688, 512, 20000)):
            for ta, tb in LAYOUT_CASES:
                both(M, N, K, ta, tb, mode, wide=1)
    out.append(_p(2688, 20000, 512, 0, 1, 1, wide=1, no_bx=1))
    # the DMA kernel: M / N / K 120 / 128, a K tail beside k- and m-contiguous operands, 256 / 257 and 1023 / 1024 tiles in the
    # weight-gradient layout, reductions around 1024 and 2560 per part, mirrors that cannot be loaded 16 bytes at a time
    for M, N, K in ((120, 128, 128), (128, 120, 128), (128, 128, 120), (128, 128, 128), (2688, 1000, 1032), (2048, 2048, 2047 * 2),
                    (2048, 2048, 5120), (2048 + 128, 2048, 5120), (128 * 1023, 128, 256), (128 * 1024, 128, 256), (1024, 1536, 5120),
                    (2688, 1024, 20000)):
        for ta, tb in LAYOUT_CASES:
            both(M, N, K, ta, tb, 1, wide=1, a16=1, b16=1)
    for kw in (dict(a16=1), dict(b16=1), dict(a16=1, b16=1, aA16=8), dict(a16=1, b16=1, lda=1028), dict(a16=1, b16=1, no_g16=1),
               dict(a16=1, b16=1, g16_cfg=643), dict(a16=1, b16=1, g16_cfg=843)):
        out.append(_p(2688, 1000, 1024, 0, 1, 1, wide=1, **kw))
    # operands the vector kernels cannot load: base, pitch, extent
    for kw in (dict(aA=4), dict(aB=8), dict(lda=1001), dict(ldb=1002)):
        for ta, tb in LAYOUT_CASES:
            both(2688, 512, 1000, ta, tb, **kw)
            out.append(_p(2688, 512, 1000, ta, tb, 3, wide=1, **kw))
    for ta, tb in LAYOUT_CASES:
        out.append(_p(2690, 514, 1001, ta, tb, cs=ta)); out.append(_p(2690, 514, 1001, ta, tb, 1, wide=1, a16=1, b16=1))
    out.append(_p(512, 512, 512, 0, 1, cs=1))      # column sums outside the weight-gradient layout: refused
    return out


# tests/test_gpu_gemm_routes.py: per family the cheapest shape its `cheapest` fixture finds -- (planner input of the public entry, bias,
# (M, N, K), the layouts the planner routes to the family).  tests/test_gemm_routes_cpu.py recomputes this table from the planner.
ENTRY_INPUTS = {"xg_gemm": dict(mode=0), "xg_gemm_mode_3": dict(mode=3, wide=1), "xg_gemm_mode_1": dict(mode=1, wide=1),
                "xg_gemm_bf16_operands": dict(mode=1, wide=1, a16=1, b16=1)}
CHEAPEST = {
    "gemm_kernel": ("xg_gemm", 1, (1, 5, 7), [(0, 1), (0, 0), (1, 0), (1, 1)]),
    "gemm_bs3": ("xg_gemm_mode_3", 1, (1, 5, 7), [(0, 1), (0, 0), (1, 0), (1, 1)]),
    "gemm_bs1": ("xg_gemm_mode_1", 1, (1, 5, 7), [(0, 1), (0, 0), (1, 0), (1, 1)]),
    "gemm_bx": ("xg_gemm_mode_1", 1, (256, 128, 64), [(0, 1), (0, 0)]),
    "g16": ("xg_gemm_bf16_operands", 1, (136, 264, 200), [(0, 0), (1, 0), (1, 1)]),
    "gemm_w1": ("xg_gemm", 1, (384, 2504, 512), [(0, 1), (0, 0), (1, 0), (1, 1)]),
    "gemm_td": ("xg_gemm", 0, (3000, 3000, 256), [(1, 0)]),
    "gemm_pk": ("xg_gemm", 1, (1280, 512, 20000), [(0, 1), (0, 0), (1, 0), (1, 1)]),
}
# the cheapest shape of gemm_kernel / gemm_bs1 / gemm_bs3 loads scalars (gemm_kernel: column sums in a separate pass; gemm_bs*: the one-row
# branch of its column sums); this one takes 16-byte loads, the branch the model's shapes take, with M % 128 == 32
COLSUM_VECTOR_SHAPE = (160, 64, 96)
COLSUM_VECTOR_FAMILIES = ("gemm_kernel", "gemm_bs1", "gemm_bs3")


def row_lengths(e):
    """(A, B, C) row lengths in elements: the pitch an input has where it names none"""
    return (e["M"] if e["ta"] else e["K"], e["K"] if e["tb"] else e["N"], e["N"])


def pitched_inputs():
    """The cheapest shape of every family (CHEAPEST), in every layout the family takes, as the model hands the library its
    sub-blocks: pitches padded by 4 and by 8 elements (rows stay 16-byte loadable), by 1 (lda / ldb: the scalar-load kernels; ldc: a
    tail rectangle that cannot be cleared, gemm_td refused), operands off the 16-byte grid -- and, in the weight-gradient layout,
    the column sums into one, two and three accumulators (`cs` = their number) with M % 128 == 32, so that the clamped rows of the
    last tile row have to stay out of the sums."""
    out = []
    for family in FAMILIES:
        entry, bias, (M, N, K), layouts = CHEAPEST[family]
        for ta, tb in layouts:
            e = _p(M, N, K, ta, tb, bias=bias, **{k: v for k, v in ENTRY_INPUTS[entry].items()})
            la, lb, lc = row_lengths(e)
            for pad in (4, 8):
                out.append(dict(e, lda=la + pad, ldb=lb + pad, ldc=lc + pad))
            out.append(dict(e, lda=la + 1, ldb=lb + 1))
            out.append(dict(e, ldc=lc + 1))
            out += [dict(e, aA=4), dict(e, aB=8), dict(e, aC=4)]
            if (ta, tb) == (1, 0):
                shapes = [(M + (32 - M) % 128, N, K)] + ([COLSUM_VECTOR_SHAPE] if family in COLSUM_VECTOR_FAMILIES else [])
                out += [dict(e, M=m, N=n, K=k, bias=0, acc=1, cs=ncs) for m, n, k in shapes for ncs in (1, 2, 3)]
    return out


VARIANT_FIELDS = ("rc", "family", "bm", "bn", "bk", "ta", "tb", "vec", "fast", "a16", "b16", "split", "clear", "colsum", "ring", "cfg",
                  "pad_lds", "relu", "acc", "bias", "rounds", "tail", "padded", "ncs")


def variant(e, route):
    """What selects a template instance or a distinct code path inside a kernel: the key under which two table inputs run the same
    code.  `route`: the planner's route of `e` as a dict of the recorded table's keys.  Fields: VARIANT_FIELDS."""
    padded = any(e.get(k, 0) not in (0, n) for k, n in zip(("lda", "ldb", "ldc"), row_lengths(e)))
    return (route["rc"], route["family"], route["bm"], route["bn"], route["bk"], e["ta"], e["tb"], route["vec"], route["fast"],
            route["a16"], route["b16"], int(route["splitk"] > 1), route["clear"], route["colsum"], route["ring"], route["cfg"],
            route["pad_lds"], e.get("relu", 0), e.get("acc", 0), e.get("bias", 0), int(route["rounds"] > 0), int(route["tail_wgs"] > 0),
            int(padded), e.get("cs", 0))


def variant_cases(golden):
    """{variant: input} over the recorded table: per variant the input with the fewest M * N * K (ties: the smaller key(e))"""
    best = {}
    for e in table_inputs():
        v = variant(e, dict(zip(golden["keys"], golden["routes"][key(e)])))
        rank = (e["M"] * e["N"] * e["K"], key(e))
        if v not in best or rank < best[v][0]:
            best[v] = (rank, e)
    return {v: e for v, (_, e) in best.items()}


def table_inputs():
    """every input of the recorded table, each once, in a fixed order"""
    seen, out = set(), []
    for e in [e for v in gpu_test_inputs().values() for e in v] + policy_inputs() + threshold_inputs() + pitched_inputs():
        if key(e) not in seen:
            seen.add(key(e))
            out.append(e)
    return out
