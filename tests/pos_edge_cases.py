"""TEST INFRASTRUCTURE ONLY -- the POS generator's edge cases (tests/test_gpu_pos_edges.py) and, as a plain function of the dims,
the host-side conditions under which each kernel branch of the POS entry points runs (tests/test_pos_edges_cpu.py checks that the
named cases reach every branch, so that an edit of the case list cannot silently drop one).

Branches (rows of the table in the docstring of tests/test_gpu_pos_edges.py):
   1  pos_attn_kernel<false>: scalar loads of v2a(V) (eval)
   2  pos_attn_kernel without the V prefetch: the context summed from memory over the `red` parts (eval)
   3  R > STEP_TPB: the j-loops of the per-video cell kernels take a second pass (eval and train)
   4  the serial head of the eval cell: one thread computes log-sum-exp and the greedy argmax (eval)
   5  the 64-wide chunk loops of the train cell and its backward: C > 64 ("5"), several chunks C > 128 ("5b") (train)
   6  the strided row loop of pos_first_zero_col_kernel (eval: T' and n; train: T')
   7  the decoder-step products on the skinny launcher's LDS-staged kernel (sk_kernel) instead of the packed fast kernel
   8  BatchNorm train forward: bn_train_fwd_kernel<20> ("8a") and the xgk_bn_stats + xgk_bn_apply fallback at R % 16 == 0 ("8b")
   9  attention train forward generic attn_fwd_kernel ("9a"); backward <48> forms ("9b") and the generic attn_bwd_kernel ("9c")
  10  xgk_attn_post_dV's two-pass path (attn_dV_kernel + attn_bwd_post_kernel<0>) at Tp > 32 (train)
"""
from __future__ import annotations

import numpy as np

# csrc/xg_pos.hip: STEP_TPB, POS_TPB; csrc/xg_attn.hip: FT
STEP_TPB, POS_TPB, ATTN_FT = 1024, 256, 1024

# name -> dims (F1 / F2 small: no branch here depends on them)
EDGE_CASES = {
    "a_odd": dict(B=3, K=5, R=20, A=30, E=10, C=6, L=5),
    "r_odd": dict(B=4, K=6, R=30, A=44, E=17, C=7, L=6),
    "k40_r512": dict(B=3, K=40, R=512, A=1536, E=468, C=20, L=6),
    "k300_r64": dict(B=2, K=300, R=64, A=96, E=36, C=20, L=4),
    "r1040": dict(B=2, K=5, R=1040, A=72, E=20, C=9, L=4),
    "c64": dict(B=5, K=7, R=40, A=52, E=24, C=64, L=7),
    "c65": dict(B=5, K=7, R=40, A=52, E=24, C=65, L=7),
    "c130": dict(B=5, K=7, R=40, A=52, E=24, C=130, L=7),
    "a2100": dict(B=2, K=6, R=32, A=2100, E=12, C=8, L=4),
    "bn20": dict(B=160, K=30, R=16, A=20, E=8, C=5, L=3),
    "bnbig": dict(B=200, K=30, R=16, A=20, E=8, C=5, L=3),
    "b300": dict(B=300, K=3, R=16, A=20, E=8, C=5, L=5),
    "t40": dict(B=3, K=6, R=32, A=40, E=12, C=8, L=39),
    "min": dict(B=1, K=1, R=8, A=4, E=4, C=2, L=1),
}
FEATS = dict(F1=20, F2=12)


def case_dims(name):
    return dict(EDGE_CASES[name], **FEATS)


def case_variant(i, d):
    """(ragged, p) of the i-th case: every other case ragged and at p = 0.5 (hash masks) -- ragged only where make_inputs can
    make it so (K >= 2 and L >= 2)."""
    alt = bool(i % 2)
    return alt and d["K"] >= 2 and d["L"] >= 2, 0.5 if alt else 0.0


def fuzz_dims(i):
    """Seeded random extents drawn from pools that hold the edges above (R > 1024, R % 4, A % 4, A > 2048, K > 32 / 48, C > 64 /
    128, B = 1 and B > 32, L >= 32)."""
    rng = np.random.RandomState(2000 + i)
    return dict(B=int(rng.choice([1, 3, 9, 33])), K=int(rng.choice([1, 2, 7, 17, 33, 40, 70])),
                R=int(rng.choice([8, 20, 30, 64, 72, 520, 1040])), A=int(rng.choice([4, 30, 96, 260, 2100])),
                E=int(rng.choice([4, 10, 36])), C=int(rng.choice([2, 5, 20, 64, 65, 130])), L=int(rng.choice([1, 3, 9, 33])),
                F1=int(rng.choice([4, 20, 48])), F2=int(rng.choice([4, 12, 40])))


# fuzz cases with the EOS weights (pos_oracle.make_params(eos=True): greedy exits early), one in four: those where some row
# survives the first choice under them (11: n = 3 of 33 steps, with the serial head)
FUZZ_EOS = (1, 6, 11)


def fuzz_variant(i, d):
    """(ragged, p, eos) of fuzz case i: every other ragged, every third with dropout, FUZZ_EOS with the EOS weights."""
    return bool(i % 2) and d["K"] >= 2 and d["L"] >= 2, 0.5 if i % 3 == 0 else 0.0, i in FUZZ_EOS


def _cdiv(a, b):
    return (a + b - 1) // b


def branches(d, mode, Tp=None):
    """The kernel branches a call at dims `d` (B K R A E C L) takes; `mode` "eval" (xgp_forward_tf + xgp_sample_greedy) or
    "train" (xgpt_forward_train + xgpt_backward over Tp steps; default T = L + 1).  A restatement of the launchers' host-side
    selection; the comments name what each condition mirrors."""
    B, K, R, A, C, L = d["B"], d["K"], d["R"], d["A"], d["C"], d["L"]
    T = L + 1
    Tp = T if Tp is None else Tp
    out = set()
    if R % 4:                                   # xg_step.hip xgk_skinny: vec needs K % 4 == 0 (K = R for the step products)
        out.add("7")
    if R > STEP_TPB:                            # xg_pos.hip: `for (int j = tid; j < R; j += STEP_TPB)` in every cell kernel
        out.add("3")
    if B > POS_TPB:                             # xg_pos.hip pos_first_zero_col_kernel: `for (b = threadIdx.x; b < B; b += POS_TPB)`
        out.add("6")
    if mode == "eval":
        if A % 4:                               # xg_pos.hip step_plan: `A % 4 == 0`
            out.add("1")
        nsplit = min(max(STEP_TPB // R, 1), K)  # xg_pos.hip step_plan: nsplit
        if not (nsplit * R <= STEP_TPB and _cdiv(K, nsplit) <= 16):     # pos_attn_kernel: `vpre`
            out.add("2")
        if C > 64:                              # pos_cell_head_kernel: `if (C <= 64) ... else if (tid == 0)`
            out.add("4")
        return out
    if C > 64:                                  # pos_cell_head_train_kernel / _bwd_kernel: `for (c0 = 0; c0 < C; c0 += 64)`
        out.add("5")
    if C > 128:
        out.add("5b")
    BK = B * K                                  # xg_pointwise.hip xgk_bn_train_fwd: R % 16, N <= 16 * 256 / 20 * 256
    if R % 16 == 0 and 16 * 256 < BK <= 20 * 256:
        out.add("8a")
    if R % 16 == 0 and BK > 20 * 256:
        out.add("8b")
    fwd_fast = False                            # xg_attn.hip xgk_attn_fwd (half_cu false)
    if A % 4 == 0 and A <= 2048 and R % 4 == 0 and 4 <= R <= 4 * ATTN_FT:
        r4n = R // 4
        nkp = min(ATTN_FT // r4n, K) if ATTN_FT // r4n > 0 else 1
        fwd_fast = K <= 16 * nkp and (((K + 3) & ~3) + nkp * R) * 4 <= 60000
    if not fwd_fast:
        out.add("9a")
    bwd_fast = A % 4 == 0 and A <= 2 * ATTN_FT and R % 4 == 0 and R <= 1024 and K <= 48      # xgk_attn_bwd (lddaf = R)
    if bwd_fast and K > 32:
        out.add("9b")
    if not bwd_fast:
        out.add("9c")
    if Tp > 32:                                 # xg_attn.hip xgk_attn_post_dV: `if (T > 32 || ...)`
        out.add("10")
    return out


# the branches each mode can reach
EVAL_ROWS = {"1", "2", "3", "4", "6", "7"}
TRAIN_ROWS = {"3", "5", "5b", "6", "7", "8a", "8b", "9a", "9b", "9c", "10"}
