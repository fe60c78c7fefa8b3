"""GPU parity tests: the HIP path (through the C ABI) vs the oracle on the same seeded inputs and vs
the golden fixtures recorded from the reference.  fp32 tolerances are written at each assert;
token streams are compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import gemm_shapes as gs
from tests.util import CFG, WEIGHT_CLASS, ZERO_GRAD_PARAMS, assert_grads_close, load_golden, make_model, oracle_grads, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    import __graft_entry__ as ge
    ge.build()


# ---------------------------------------------------------------- GEMM building block
@pytest.mark.parametrize("M,N,K", gs.LAYOUTS)
@pytest.mark.parametrize("ta,tb", gs.LAYOUT_CASES)
def test_gemm_layouts(M, N, K, ta, tb):
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + ta * 2 + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    Bm = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    ref = (A.t() if ta else A).double() @ (Bm.t() if tb else Bm).double()
    Ad, Bd, bd = A.cuda(), Bm.cuda(), bias.cuda()
    for relu, acc in ((0, 0), (1, 0), (0, 1)):
        Cd = C0.clone().cuda()
        rc = L.xg_gemm(None, ta, tb, M, N, K, nv.ptr(Ad), A.shape[1], nv.ptr(Bd), Bm.shape[1], nv.ptr(Cd), N, nv.ptr(bd),
                       relu, acc)
        assert rc == 0
        want = ref + bias.double() + (C0.double() if acc else 0)
        if relu:
            want = want.clamp(min=0)
        got = Cd.cpu().double()
        tol = 2e-6 * np.sqrt(K) * 4 + 1e-6          # fp32 fmaf chain: |err| ~ 1e-7 * sum|a*b|
        assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (relu, acc)


@pytest.mark.parametrize("M,N,K", gs.PERSISTENT)
@pytest.mark.parametrize("ta,tb", gs.LAYOUT_CASES)
def test_gemm_persistent_kernel_shapes(M, N, K, ta, tb):
    """Shapes large enough for the persistent 128x128 kernel (whole-tile rounds + stream-K tail with atomics, partial last
    slab, ragged edges, ReLU without splitting, += C): every element of C against fp64."""
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 5 * K + ta * 2 + tb)
    Ad = torch.randn((K, M) if ta else (M, K), generator=g, device="cuda")
    Bd = torch.randn((N, K) if tb else (K, N), generator=g, device="cuda")
    bd = torch.randn(N, generator=g, device="cuda")
    C0 = torch.randn(M, N, generator=g, device="cuda")
    ref = (Ad.t() if ta else Ad).double() @ (Bd.t() if tb else Bd).double() + bd.double()
    scale = float(ref.abs().max())
    for relu, acc in ((0, 0), (1, 0), (0, 1)):
        Cd = C0.clone()
        assert L.xg_gemm(None, ta, tb, M, N, K, nv.ptr(Ad), Ad.shape[1], nv.ptr(Bd), Bd.shape[1], nv.ptr(Cd), N, nv.ptr(bd),
                         relu, acc) == 0
        want = ref + (C0.double() if acc else 0)
        if relu:
            want = want.clamp(min=0)
        err = float((Cd.double() - want).abs().max()) / scale
        assert err < 4e-6 * max(1.0, np.sqrt(K / 4096.0)), (relu, acc, err)     # fp32 chain: grows with sqrt(K)


_GEMM_FUZZ = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from controllable_xgating_amd import _native as nv
L = nv.lib()
rng = np.random.RandomState(11)
bad = []
for it in range(36):
    M = int(rng.choice([130, 257, 384, 511, 777, 1024, 1411, 2688]))
    N = int(rng.choice([128, 260, 512, 1000, 1536, 2052, 4100]))
    K = int(rng.choice([32, 96, 132, 468, 512, 1000, 2688]))
    ta, tb = int(rng.randint(2)), int(rng.randint(2))
    relu, acc = [(0, 0), (1, 0), (0, 1)][int(rng.randint(3))]
    mode = int(rng.choice([0, 0, 1, 3]))
    g = torch.Generator(device="cuda").manual_seed(1000 + it)
    A = torch.randn((K, M) if ta else (M, K), generator=g, device="cuda")
    B = torch.randn((N, K) if tb else (K, N), generator=g, device="cuda")
    b = torch.randn(N, generator=g, device="cuda")
    C0 = torch.randn(M, N, generator=g, device="cuda")
    C = C0.clone()
    assert L.xg_gemm_mode(None, mode, ta, tb, M, N, K, nv.ptr(A), A.shape[1], nv.ptr(B), B.shape[1], nv.ptr(C), N, nv.ptr(b), relu, acc) == 0
    want = (A.t() if ta else A).double() @ (B.t() if tb else B).double() + b.double() + (C0.double() if acc else 0)
    if relu:
        want = want.clamp(min=0)
    err = float((C.double() - want).abs().max()) / float(want.abs().max())
    tol = 2e-2 if mode == 1 else 6e-6
    if not err < tol:
        bad.append((it, M, N, K, ta, tb, relu, acc, mode, err))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("pk_min,bg", [("2", False), ("40", False), ("2", True)])
def test_gemm_fuzz_all_kernels(pk_min, bg):
    """36 seeded random products (ragged extents, all four layouts, bias / ReLU / += C, fp32 / bf16 / split-bf16) against fp64,
    once with the persistent stream-K kernel forced onto every shape that can take it (XG_PK_MIN=2: read at first use, hence
    the subprocess), once with the production rule, and once with the persistent kernel in its background form (one
    workgroup per CU: 256-workgroup grid, padded LDS -- what the side-stream vocabulary products of a training step use)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from controllable_xgating_amd import _native as nv
    env = dict(os.environ, XG_PK_MIN=pk_min, XG_LIBRARY=nv.LIB_DIAG_PATH)      # the switches exist in the -DXG_DIAG build only
    if bg:
        env["XG_GEMM_FORCE_BG"] = "1"
    r = subprocess.run([sys.executable, "-c", _GEMM_FUZZ % root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


_GEMM_W1 = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from controllable_xgating_amd import _native as nv
from tests.gemm_shapes import W1_SHAPES
L = nv.lib()
bad = []
for (M, N, K) in W1_SHAPES:
    for ta, tb in ((0, 1), (0, 0), (1, 0), (1, 1)):
        g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 5 * K + ta * 2 + tb)
        A = torch.randn((K, M) if ta else (M, K), generator=g, device="cuda")
        B = torch.randn((N, K) if tb else (K, N), generator=g, device="cuda")
        b = torch.randn(N, generator=g, device="cuda")
        C0 = torch.randn(M, N, generator=g, device="cuda")
        ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double() + b.double()
        scale = float(ref.abs().max())
        for relu, acc in ((0, 0), (1, 0), (0, 1)):
            Cd = C0.clone()
            rc = L.xg_gemm(None, ta, tb, M, N, K, nv.ptr(A), A.shape[1], nv.ptr(B), B.shape[1], nv.ptr(Cd), N, nv.ptr(b), relu, acc)
            want = ref + (C0.double() if acc else 0)
            if relu: want = want.clamp(min=0)
            err = float((Cd.double() - want).abs().max()) / scale
            if rc != 0 or not err < 4e-6: bad.append((M, N, K, ta, tb, relu, acc, rc, err))
print("bad", bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("tile", gs.W1_TILE_CASES)
def test_gemm_one_workgroup_per_cu_kernel(tile):
    """xg_gemm.hip's deep-slab kernel for products of about one round of tiles (gemm_w1_kernel: two register sets of global
    loads, MFMAs interleaved with the LDS / global instructions): every tile shape forced onto ragged products (XG_W1_TILE of the
    -DXG_DIAG library; rows / columns past the edge, one and several rounds of workgroups, 2-12 slabs), all four layouts,
    bias / ReLU / += C, every element against fp64; "auto" = the production rule on the same shapes."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from controllable_xgating_amd import _native as nv
    env = dict(os.environ, XG_LIBRARY=nv.LIB_DIAG_PATH)
    if tile != "auto":
        env["XG_W1_TILE"] = tile
    r = subprocess.run([sys.executable, "-c", _GEMM_W1 % root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_rollout_token_choice_over_tile_statistics_equals_the_row_pass():
    """Rollout steps of <= 128 rows take xg_heads.hip's vocab_part_kernel (vocabulary product + per-tile row statistics, logits
    stored for the sampled / replayed rows only) and roll_select_kernel (token choice over the statistics); the older (B, V)
    product + one-workgroup-per-row pass stays for every other shape.  Same paired SCST rollout (sampled half with temperatures
    0.7 / 1 / 1.3, greedy half), a replay of its tokens and the SCST backward through both: tokens identical, log-probs and
    gradient norms to fp32 round-off, on vocabularies that are / are not multiples of the 32-column tile (tools/select_check.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "select_check.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bad []" in r.stdout, r.stdout[-2500:] + r.stderr[-2500:]


@pytest.mark.parametrize("rows", [40, 128])
def test_dataflow_step_kernel_equals_three_launch_step(rows):
    """xg_dstep.hip (the decoder step as ONE dataflow launch: measurement-only, selected with XG_DSTEP=1 in the -DXG_DIAG
    library) against the product's three-launch step: three chained in-place xg_step_fwd calls on the same inputs, state and
    attention weights equal to fp32 round-off (tools/dstep_check.py; 40 rows = a ragged second m-tile)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "dstep_check.py")], env=dict(os.environ, DS_B=str(rows)),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "us per step" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


_GEMM_TD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from controllable_xgating_amd import _native as nv
from tests.gemm_shapes import TD_SHAPES
L = nv.lib()
bad = []
for (M, N, K) in TD_SHAPES:
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 5 * K)
    A = torch.randn(K, M, generator=g, device="cuda")
    B = torch.randn(K, N, generator=g, device="cuda")
    C0 = torch.randn(M, N, generator=g, device="cuda")
    ref = A.t().double() @ B.double()
    scale = float(ref.abs().max())
    for acc in (0, 1):
        Cd = C0.clone()
        rc = L.xg_gemm(None, 1, 0, M, N, K, nv.ptr(A), M, nv.ptr(B), N, nv.ptr(Cd), N, None, 0, acc)
        want = ref + (C0.double() if acc else 0)
        err = float((Cd.double() - want).abs().max()) / scale
        if rc != 0 or not err < 4e-6 * max(1.0, np.sqrt(K / 4096.0)): bad.append((M, N, K, acc, rc, err))
print("bad", bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("rule", list(gs.TD_RULES))
def test_gemm_weight_gradient_layout_from_memory(rule):
    """C (+)= A^T B with both operands stored (K, .): xg_gemm.hip's gemm_td_kernel (v_mfma_f32_16x16x4_f32 fed by 16-byte global loads
    in the instruction's own operand layout, no LDS image; four waves per 64 x 64 tile on interleaved k-steps, added through LDS;
    a cross-workgroup split of the reduction with atomics when there are few tiles; persistent rounds when there are many).
    Ragged edges (extents that are multiples of 4 but not of 64), plain store and += C, every element against fp64.  The
    production rule sends only the vocabulary head's weight gradient there (20000 x 512: see xg_gemm_route.h, plan_td); the -DXG_DIAG library's
    XG_TD_ALL=1 every eligible product (few tiles: split reductions; XG_TD_KS / XG_TD_DEPTH force the split and the ring depth)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from controllable_xgating_amd import _native as nv
    env = dict(os.environ)
    if rule != "production":
        env.update(XG_LIBRARY=nv.LIB_DIAG_PATH, XG_TD_ALL="1")
    if rule == "split_2":
        env["XG_TD_KS"] = "2"
    if rule == "depth_4":
        env["XG_TD_DEPTH"] = "4"
    r = subprocess.run([sys.executable, "-c", _GEMM_TD % root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_gemm_strided_submatrix():
    """W[:, R:2R] column block of h2a.weight as B operand (ldb = 2R) and accumulate, as the step uses it."""
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g = torch.Generator().manual_seed(5)
    B_, R, A = 16, 64, 96
    h = torch.randn(B_, R, generator=g); W = torch.randn(A, 2 * R, generator=g); P0 = torch.randn(B_, A, generator=g)
    hd, Wd, Pd = h.cuda(), W.cuda(), P0.clone().cuda()
    rc = L.xg_gemm(None, 0, 1, B_, A, R, nv.ptr(hd), R, C.c_void_p(Wd.data_ptr() + 4 * R), 2 * R, nv.ptr(Pd), A, None, 0, 1)
    assert rc == 0
    want = P0 + h @ W[:, R:].t()
    assert float((Pd.cpu() - want).abs().max()) < 1e-4


# ---------------------------------------------------------------- XE forward / backward
def run_oracle_xe(d, ragged, p=0.0, seed=0, train=True, weight_class=WEIGHT_CLASS):
    P = xo.to_torch_params(pg.make_params(d), requires_grad=True)
    x = xo.to_torch_inputs(pg.make_inputs(d, seed=0, ragged=ragged))
    running = xo.new_running(d)
    logp, cat, V = xo.forward_xe(P, x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"],
                                 x["seq_mask"], train=train, p=p, seed=seed, running=running)
    l_xe = xo.lm_criterion(logp, x["seq"], x["seq_mask"])
    l_cls = xo.cls_criterion(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    loss = l_xe + weight_class * l_cls
    loss.backward()
    return P, logp.detach().numpy(), cat.detach().numpy(), l_xe.item(), l_cls.item(), running


def run_hip_xe(d, ragged, p=0.0, seed=None, weight_class=WEIGHT_CLASS, precision="fp32"):
    from controllable_xgating_amd import ClassiferCriterion, LanguageModelCriterion
    model = make_model(d, p_drop=p, precision=precision)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=ragged))
    if seed is not None:
        model.dropout_seed = seed
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    l_xe = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    l_cls = ClassiferCriterion()(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    loss = l_xe + weight_class * l_cls
    loss.backward()
    torch.cuda.synchronize()
    return model, logp.detach().cpu().numpy(), cat.detach().cpu().numpy(), l_xe.item(), l_cls.item()


@pytest.mark.parametrize("tag,ragged", [("tiny", False), ("tiny", True), ("odd", True), ("one", False), ("mid", True), ("c1", False),
                                        ("c1", True)])
def test_xe_forward_backward_vs_oracle(tag, ragged):
    d = pg.make_dims(**CFG[tag])
    P, lo, co, lxe_o, lcls_o, running = run_oracle_xe(d, ragged)
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, ragged)
    assert abs(lxe_h - lxe_o) < 1e-4, (lxe_h, lxe_o)            # north_star: training loss within 1e-4 (fp32)
    assert abs(lcls_h - lcls_o) < 1e-4
    np.testing.assert_allclose(lh, lo, atol=3e-4, rtol=0)
    np.testing.assert_allclose(ch, co, atol=1e-4, rtol=0)
    assert_grads_close(model, oracle_grads(P))
    enc = model.two_spatial_encoder
    for mod in ("rgb", "opfl"):
        bn = getattr(enc, f"visual_emb_{mod}")[1]
        pre = xo.ENC + f"visual_emb_{mod}.1."
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), running[pre + "running_mean"].numpy(), atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), running[pre + "running_var"].numpy(), atol=1e-5)


@pytest.mark.parametrize("tag,ragged", [("tiny", True), ("c1", False), ("c1", True)])
def test_xe_vs_reference_golden(tag, ragged):
    g = load_golden(f"xe_{tag}{'_ragged' if ragged else ''}.npz")
    d = pg.make_dims(**CFG[tag])
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, ragged)
    assert abs(lxe_h - float(g["loss_xe"])) < 1e-4
    assert abs(lcls_h - float(g["loss_cls"])) < 1e-4
    ns = g["logp_slice"].shape[2]
    np.testing.assert_allclose(lh[:, :, :ns], g["logp_slice"], atol=3e-4, rtol=0)
    for name, prm in model.named_parameters():
        gr = prm.grad.cpu().numpy()
        gn = np.sqrt((gr.astype(np.float64) ** 2).sum())
        ref_n = float(g["gnorm/" + name])
        assert abs(gn - ref_n) <= 2e-3 * ref_n + 1e-6, (name, gn, ref_n)


def test_fused_xe_loss_path_equals_surface_path():
    """xg_xe_loss_fwd/bwd (no (m,T,V) gradient tensor) == model() + criteria + backward."""
    d = pg.make_dims(**CFG["mid"])
    P, lo, co, lxe_o, lcls_o, _ = run_oracle_xe(d, True)
    model = make_model(d)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"],
                         x["cap_classes"], x["class_mask"], WEIGHT_CLASS)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - (lxe_o + WEIGHT_CLASS * lcls_o)) < 1e-4
    ll = model.last_losses.cpu().numpy()
    assert abs(ll[1] - lxe_o) < 1e-4 and abs(ll[2] - lcls_o) < 1e-4
    assert_grads_close(model, oracle_grads(P))


def test_dropout_masks_match_oracle_hash():
    """p = 0.5 in train mode: HIP regenerates exactly the oracle's integer-hash masks."""
    d = pg.make_dims(**CFG["mid"])
    seed = 123457
    P, lo, co, lxe_o, lcls_o, _ = run_oracle_xe(d, True, p=0.5, seed=seed)
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, True, p=0.5, seed=seed)
    assert abs(lxe_h - lxe_o) < 2e-4, (lxe_h, lxe_o)
    np.testing.assert_allclose(lh, lo, atol=5e-4, rtol=0)
    assert_grads_close(model, oracle_grads(P), rtol=3e-3)


def test_eval_mode_batchnorm_vs_golden(p_drop=0.0):
    g = load_golden("evalbn_c1.npz")
    d = pg.make_dims(**CFG["c1"])
    model = make_model(d, train=False, p_drop=p_drop)
    enc = model.two_spatial_encoder
    for mod in ("rgb", "opfl"):
        bn = getattr(enc, f"visual_emb_{mod}")[1]
        bn.running_mean.copy_(torch.from_numpy(pg.uniform(f"rm.{mod}", (d.R,), 9, -0.3, 0.3)))
        bn.running_var.copy_(torch.from_numpy(pg.uniform(f"rv.{mod}", (d.R,), 9, 0.5, 2.0)))
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    from controllable_xgating_amd import LanguageModelCriterion
    with torch.no_grad():
        logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
        loss = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    np.testing.assert_allclose(logp.cpu().numpy()[:, :, :32], g["logp_slice"], atol=3e-4)


# ---------------------------------------------------------------- single step / state surface
def test_single_step_vs_reference_golden():
    g = load_golden("step_c1.npz")
    cfg = dict(CFG["c1"]); cfg["B"] = 4
    d = pg.make_dims(**cfg)
    model = make_model(d, train=True)
    B, K, R, E = d.B, d.K, d.R, d.E
    V = torch.from_numpy(pg.uniform("step.V", (B, K, R), 5, 0.0, 1.0)).cuda()
    pos = torch.from_numpy(pg.uniform("step.pos", (B, R), 5, -1.0, 1.0)).cuda()
    st = [torch.from_numpy(pg.uniform(f"step.s{i}", (1, B, R), 5, -0.5, 0.5)).cuda() for i in range(4)]
    # the golden drives lstmcore with an arbitrary xt: plant it as the embedding rows of tokens 2..5
    xt = torch.from_numpy(pg.uniform("step.xt", (B, E), 5, -0.1, 0.1)).cuda()
    with torch.no_grad():
        model.embed.weight[2:2 + B].copy_(xt)
    it = torch.arange(2, 2 + B, device="cuda")
    logp, state = model.get_logprobs_state(it, V, pos, [(st[0], st[1]), (st[2], st[3])])
    torch.cuda.synchronize()
    # get_logprobs_state uses a mask of ones (SAModel.py:121): compare the unmasked rows 0,1,3
    rows = [0, 1, 3]
    np.testing.assert_allclose(state[0][0][0].cpu().numpy()[rows], g["h1"][rows], atol=2e-5)
    np.testing.assert_allclose(state[0][1][0].cpu().numpy()[rows], g["c1"][rows], atol=2e-5)
    np.testing.assert_allclose(state[1][0][0].cpu().numpy()[rows], g["h2"][rows], atol=2e-5)
    np.testing.assert_allclose(state[1][1][0].cpu().numpy()[rows], g["c2"][rows], atol=2e-5)


def test_init_hidden_and_encoder_surface():
    d = pg.make_dims(**CFG["mid"])
    model = make_model(d)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    V = model.encode(x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    st = model.init_hidden(V, x["feat_mask"])
    P = xo.to_torch_params(pg.make_params(d))
    xi = xo.to_torch_inputs(pg.make_inputs(d, seed=0, ragged=True))
    Vo = xo.encoder_fwd(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], train=True, running=xo.new_running(d))
    so = xo.init_hidden(P, Vo, xi["feat_mask"])
    np.testing.assert_allclose(V.cpu().numpy(), Vo.numpy(), atol=2e-5)
    assert st[0][0].shape == (1, d.B, d.R)
    np.testing.assert_allclose(st[0][0][0].cpu().numpy(), so[0][0].numpy(), atol=2e-5)
    np.testing.assert_allclose(st[1][1][0].cpu().numpy(), so[1][1].numpy(), atol=2e-5)


# ---------------------------------------------------------------- rollouts
@pytest.mark.parametrize("name,tag,ragged", [("greedy_tiny.npz", "tiny", False), ("greedy_c1.npz", "c1", False),
                                              ("greedy_c1_ragged.npz", "c1", True)])
def test_greedy_token_for_token_vs_reference(name, tag, ragged, p_drop=0.0):
    g = load_golden(name)
    d = pg.make_dims(**CFG[tag])
    assert float(g["min_margin"]) >= 1e-3                  # the reference's own top-2 margins, recorded in the fixture
    model = make_model(d, P=pg.make_params(d, logit_gain=float(g["logit_gain"])), train=False, p_drop=p_drop)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=ragged))
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    seq, slp = seq.cpu().numpy(), slp.cpu().numpy()
    assert seq.shape == g["seq"].shape
    # a flip is only tolerated where the reference's own top-1/top-2 margin is below fp32 noise (none expected)
    diff = seq != g["seq"]
    assert not diff.any(), (np.argwhere(diff), g["margin"].min())
    np.testing.assert_allclose(slp, g["seqLogprobs"], atol=3e-4)


def test_rollouts_on_unaligned_dims_generic_path():
    """R % 8 != 0 and nothing 16-byte aligned: the generic (non-skinny) step path; greedy tokens + replay gradients."""
    from controllable_xgating_amd import RewardCriterion
    d = pg.make_dims(**CFG["odd"])
    model = make_model(d, train=False)
    x = to_dev(pg.make_inputs(d, seed=0))
    xi = xo.to_torch_inputs(pg.make_inputs(d, seed=0))
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
        so, lo = xo.sample(xo.to_torch_params(pg.make_params(d)), xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"],
                           xi["pos_feats"], d.L, mode="greedy", train=False, running=xo.new_running(d))
    assert np.array_equal(seq.cpu().numpy(), so.numpy())
    np.testing.assert_allclose(slp.cpu().numpy(), lo.numpy(), atol=3e-4)
    model.train()
    forced = torch.from_numpy(pg.randint("odd.forced", (d.B, d.L), 3, 1, d.V)).cuda()
    seq2, slp2 = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 0, "forced_tokens": forced})
    reward = torch.from_numpy(pg.uniform("odd.rew", (d.B, d.L), 3, -1, 1)).cuda()
    RewardCriterion()(slp2, seq2, reward).backward()
    P = xo.to_torch_params(pg.make_params(d), requires_grad=True)
    s3, l3 = xo.sample(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L, mode="replay",
                       forced=forced.cpu(), train=True, running=xo.new_running(d))
    xo.reward_criterion(l3, s3, reward.cpu()).backward()
    torch.cuda.synchronize()
    assert_grads_close(model, oracle_grads(P))


def test_greedy_all_rows_finish_at_first_step():
    """Edge case: EOS wins at t = 1 for every row -> n = 0 (the reference would fail in torch.cat on an
    empty list, SAModel.py:219; the HIP path returns empty (m,0) tensors like the oracle)."""
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d)
    Pn["logit.bias"] = Pn["logit.bias"].copy(); Pn["logit.bias"][0] += 6.0
    model = make_model(d, P=Pn, train=False)
    x = to_dev(pg.make_inputs(d, seed=0))
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    assert tuple(seq.shape) == (d.B, 0) and tuple(slp.shape) == (d.B, 0)


@pytest.mark.parametrize("tag", ["tiny", "c1"])
def test_scst_replay_vs_reference_golden(tag):
    from controllable_xgating_amd import RewardCriterion
    g = load_golden(f"scst_{tag}.npz")
    d = pg.make_dims(**CFG[tag])
    model = make_model(d, train=True)
    x = to_dev(pg.make_inputs(d, seed=0))
    forced = torch.from_numpy(g["seq"]).cuda()
    seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                            {"sample_max": 0, "forced_tokens": forced})
    n = g["seq"].shape[1]
    assert np.array_equal(seq.cpu().numpy()[:, :n], g["seq"])
    m = np.concatenate([np.ones((d.B, 1), bool), g["seq"][:, :-1] > 0], 1)
    np.testing.assert_allclose(slp.detach().cpu().numpy()[:, :n][m], g["seqLogprobs"][m], atol=3e-4)
    reward = torch.from_numpy(g["reward"]).cuda()
    loss = RewardCriterion()(slp[:, :n], seq[:, :n], reward)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    torch.cuda.synchronize()
    for name, prm in model.named_parameters():
        gr = prm.grad.cpu().numpy() if prm.grad is not None else np.zeros(tuple(prm.shape), np.float32)
        gn = np.sqrt((gr.astype(np.float64) ** 2).sum())
        ref_n = float(g["gnorm/" + name])
        assert abs(gn - ref_n) <= 3e-3 * ref_n + 1e-6, (name, gn, ref_n)
        if "gfull/" + name in g:
            np.testing.assert_allclose(gr, g["gfull/" + name], atol=2e-6 + 2e-3 * np.abs(g["gfull/" + name]).max(),
                                       err_msg=name)


def test_sampling_inverse_cdf_and_ragged_early_stop():
    """Multinomial rollout with supplied uniforms, EOS probability ~0.3 per step so rows finish at
    different steps and the loop exits early (SAModel.py:200-210): same n as the oracle, finished rows
    emit 0, and every drawn token's CDF interval (float64, from the step's own log-probs) contains its
    uniform."""
    cfg = dict(CFG["mid"]); cfg["L"] = 24
    d = pg.make_dims(**cfg)
    Pn = pg.make_params(d, logit_gain=1.0)
    Pn["logit.bias"] = Pn["logit.bias"].copy(); Pn["logit.bias"][0] += 5.4
    model = make_model(d, P=Pn, train=False)
    x = to_dev(pg.make_inputs(d, seed=0))
    T = d.L + 1
    u = torch.from_numpy(pg.uniform("uni", (T, d.B), 77)).cuda()
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                {"sample_max": 0, "uniforms": u})
    xi = xo.to_torch_inputs(pg.make_inputs(d, seed=0))
    Po = xo.to_torch_params(Pn)
    with torch.no_grad():
        s_or, _ = xo.sample(Po, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L, mode="sample",
                            uniforms=u.cpu().numpy(), train=False, running=xo.new_running(d))
        so, lo, logps = xo.sample(Po, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L,
                                  mode="replay", forced=seq.cpu(), train=False, running=xo.new_running(d), return_logp=True)
    assert 0 < seq.shape[1] < d.L, seq.shape                     # early exit happened
    assert seq.shape == s_or.shape                               # same n as the oracle's own sampler
    seqn = seq.cpu().numpy(); un = u.cpu().numpy()
    alive = np.ones(d.B, bool)
    for t in range(1, seqn.shape[1] + 1):
        lp = logps[t - 1].numpy().astype(np.float64)
        cdf = np.cumsum(np.exp(lp), axis=1); tot = cdf[:, -1]
        for b in range(d.B):
            tok = seqn[b, t - 1]
            if not alive[b]:
                assert tok == 0                                  # it * unfinished (SAModel.py:208)
                continue
            lo_ = (cdf[b, tok - 1] if tok > 0 else 0.0) / tot[b]; hi_ = cdf[b, tok] / tot[b]
            assert lo_ - 1e-4 <= un[t, b] <= hi_ + 1e-4, (t, b, tok, lo_, un[t, b], hi_)
            if tok == 0:
                alive[b] = False
    mism = (seqn != s_or.numpy()).sum()
    assert mism <= 1, mism                                       # identical up to a CDF-boundary coin flip


def test_greedy_ties_take_lowest_index():
    """torch.max tie rule (SAModel.py:186): duplicate the best logit row into a lower index."""
    d = pg.make_dims(**CFG["tiny"])
    Pn = pg.make_params(d)
    model = make_model(d, P=Pn, train=False)
    x = to_dev(pg.make_inputs(d, seed=0))
    with torch.no_grad():
        seq, _ = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    first = int(seq[0, 0])
    if first <= 2:
        pytest.skip("need a first token with room below it")
    Pn2 = {k: v.copy() for k, v in Pn.items()}
    Pn2["logit.weight"][2] = Pn2["logit.weight"][first]; Pn2["logit.bias"][2] = Pn2["logit.bias"][first]
    model2 = make_model(d, P=Pn2, train=False)
    with torch.no_grad():
        seq2, _ = model2.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    assert int(seq2[0, 0]) == 2


# ---------------------------------------------------------------- update
def test_clip_adam_matches_torch_semantics():
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g0 = torch.Generator().manual_seed(3)
    n = 100003
    p = torch.randn(n, generator=g0); g = torch.randn(n, generator=g0) * 0.3
    m = torch.zeros(n); v = torch.zeros(n)
    pd, gd, md, vd = p.clone().cuda(), g.clone().cuda(), m.clone().cuda(), v.clone().cuda()
    po, mo, vo = p.clone(), m.clone(), v.clone()
    for step in (1, 2, 3):
        assert L.xg_clip_adam(None, n, nv.ptr(pd), nv.ptr(gd), nv.ptr(md), nv.ptr(vd), 4e-4, 0.9, 0.999, 1e-8, 0.0, step, 0.1) == 0
        gc = g.clamp(-0.1, 0.1)
        po, mo, vo = xo.adam_step(po, gc, mo, vo, step, 4e-4)
    np.testing.assert_allclose(pd.cpu().numpy(), po.numpy(), atol=1e-6)
    np.testing.assert_allclose(gd.cpu().numpy(), g.clamp(-0.1, 0.1).numpy(), atol=0)


def test_overlapped_update_equals_plain_update():
    """ClipAdam(overlap=True) -- segment updates behind the library's gradient events, two of them on a side stream while
    the backward is still running -- must leave exactly the parameters / moments / (clamped) gradients of the one fused
    update after the backward: three XE iterations from the same start, element for element."""
    from controllable_xgating_amd.train import ClipAdam
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    out = []
    for overlap in (False, True):
        model = make_model(d)
        opt = ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=overlap)
        for _ in range(3):
            opt.zero_grad()
            loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
            opt.arm()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        assert getattr(model, "_grad_event", None) is None
        out.append(({n: q.detach().clone() for n, q in model.named_parameters()}, float(loss.detach())))
    (p0, l0), (p1, l1) = out
    # the weight gradients themselves carry split-K atomics (run-to-run 1e-7 noise), so two runs agree to that level --
    # except where the TRUE gradient is zero: Adam normalises pure noise there to +-lr per step in any two runs
    assert abs(l0 - l1) < 1e-5
    for n in p0:
        if n in ZERO_GRAD_PARAMS:
            continue
        assert float((p0[n] - p1[n]).abs().max()) < 5e-6, n


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_early_repack_of_the_decoder_tiles_equals_a_full_repack(precision):
    """ClipAdam(overlap=True) refreshes the packed tiles of every matrix but the CG encoder's right behind the update of their
    parameter group (SAModel.pack_early: xg_pack_weights_part, part 1, on the optimizer's side stream, under the encoder's
    backward) and the next call only packs the encoder's tiles (part 2): the shadow must be bit-identical to a full
    xg_pack_weights of the updated parameters -- and stale when the early part is skipped on purpose (the test tests something).
    bf16: the same for the bf16 tiles and the bf16 copies of the large products' weights (round 5); bf16x3: the three pre-split
    bf16 planes (packed_dtype 2, the default of split-bf16).  Also: any other writer between pack_early() and the next call
    (a plain mark_params_changed()) voids the early part -- the full re-pack runs."""
    import ctypes as C
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import train as tr
    from controllable_xgating_amd.model import _stream
    from controllable_xgating_amd.train import ClipAdam
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    model = make_model(d, precision=precision)
    opt = ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=True, fused_zero=True)
    for it in range(3):
        opt.zero_grad()
        loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
        opt.arm()
        loss.backward()
        before = model._packed.clone()
        opt.step()
        assert model._early_key is not None and model._early_epoch == model._packed_epoch       # the early part ran
        model._packed_ptr()                                   # what the next forward would do: encoder tiles only
        assert model._early_key is None
        torch.cuda.synchronize()
        two_part = model._packed.clone()
        model.mark_params_changed()
        model._packed_ptr()                                   # a full re-pack of the same parameters
        torch.cuda.synchronize()
        assert torch.equal(two_part, model._packed)
        assert not torch.equal(before, model._packed)         # (the update really changed the tiles)
    full = model._packed.clone()
    # negative control: one more update WITHOUT the early part, then only part 2 (the encoder's tiles) -> the decoder's tiles are
    # the previous step's, the shadow differs from a full pack of the updated parameters
    opt.zero_grad()
    loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    opt.arm()
    loss.backward()
    tr._NO_EARLY_PACK, keep = True, tr._NO_EARLY_PACK
    try:
        opt.step()
    finally:
        tr._NO_EARLY_PACK = keep
    assert model._early_key is None
    dt = model._packed_dtype()
    dd = model._dims(1, 1, 1)
    nbytes = nv.lib().xg_packed_bytes(C.byref(dd), dt)
    ptr = (model._packed.data_ptr() + 15) & ~15
    ps = model._params_struct()
    nv.check(nv.lib().xg_pack_weights_part(_stream(), C.byref(dd), C.byref(ps), C.c_void_p(ptr), C.c_size_t(nbytes), dt, 1, 2),
             "xg_pack_weights_part")
    torch.cuda.synchronize()
    stale = model._packed.clone()
    assert not torch.equal(stale, full)                       # (the encoder's tiles did move)
    model._packed_ptr()                                       # the model itself saw no early part: a full re-pack
    torch.cuda.synchronize()
    assert not torch.equal(stale, model._packed)              # part 2 alone left the decoder's tiles stale
    # ... and a foreign writer between pack_early() and the next call voids the early part
    opt.zero_grad()
    loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    opt.arm()
    loss.backward()
    opt.step()
    assert model._early_key is not None
    with torch.no_grad():
        model.flat_parameters().data.mul_(1.0001)             # through .data: no version counter moves
    model.mark_params_changed()
    assert model._early_key is None
    model._packed_ptr()
    torch.cuda.synchronize()
    a = model._packed.clone()
    model.mark_params_changed()
    model._packed_ptr()
    torch.cuda.synchronize()
    assert torch.equal(a, model._packed)


def test_fused_zero_grad_update_equals_plain_update():
    """ClipAdam(fused_zero=True): the update leaves .grad at zero (xg_clip_adam_zero) and the next zero_grad() is skipped --
    same parameters as the plain update over three iterations (with and without the overlapped segments); and zero_grad()
    still clears the buffer when something wrote to it after the update (a backward without a step, an in-place edit)."""
    from controllable_xgating_amd.train import ClipAdam
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    args = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    out = []
    for fused, overlap in ((False, False), (True, False), (True, True)):
        model = make_model(d)
        opt = ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=overlap, fused_zero=fused)
        for _ in range(3):
            opt.zero_grad()
            loss = model.xe_loss(*args)
            opt.arm()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        out.append({n: q.detach().clone() for n, q in model.named_parameters()})
        g = model.flat_grads()
        if fused:
            assert float(g.abs().max()) == 0.0                       # left at zero by the update itself
            v = g._version
            opt.zero_grad()
            assert g._version == v                                     # ... so zero_grad() had nothing to do
            model.xe_loss(*args).backward()                            # a backward WITHOUT a step
            assert float(g.abs().max()) > 0.0
            opt.zero_grad()
            assert float(g.abs().max()) == 0.0
            opt.zero_grad(); loss = model.xe_loss(*args); opt.arm(); loss.backward(); opt.step()
            next(model.parameters()).grad.add_(1.0)                    # an in-place edit of a .grad after the update
            opt.zero_grad()
            assert float(g.abs().max()) == 0.0
        else:
            assert 0.0 < float(g.abs().max()) <= 0.1 + 1e-7           # the reference leaves the clamped gradient
    for other in out[1:]:
        for n in out[0]:
            if n in ZERO_GRAD_PARAMS:
                continue
            assert float((out[0][n] - other[n]).abs().max()) < 5e-6, n


# ---------------------------------------------------------------- beam search
@pytest.mark.parametrize("tag", ["tiny", "c1"])
def test_beam_search_vs_reference_golden(tag, p_drop=0.0):
    g = load_golden(f"beam_{tag}.npz")
    cfg = dict(CFG[tag]); cfg["B"] = min(cfg["B"], 3)
    d = pg.make_dims(**cfg)
    model = make_model(d, train=False, p_drop=p_drop)
    x = to_dev(pg.make_inputs(d, seed=0))
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                {"beam_size": int(g["beam_size"])})
    assert np.array_equal(seq.cpu().numpy(), g["seq"]), (seq, g["seq"])
    np.testing.assert_allclose(slp.cpu().numpy(), g["seqLogprobs"], atol=3e-4)
    assert len(model.done_beams) == d.B and len(model.done_beams[0]) >= 1


# ---------------------------------------------------------------- driver counterpart
@pytest.mark.parametrize("beam", [1, 3])
def test_eval_split_vs_oracle_and_beam_golden(beam, p_drop=0.0):
    """eval_utils.eval_split (eval_utils.py:18-84): eval-mode loss = language + weight_class * category loss per batch,
    averaged over batches; captions = decoded greedy tokens (oracle) or beam-search tokens (reference golden); the model
    is back in train mode afterwards."""
    from controllable_xgating_amd import ClassiferCriterion, LanguageModelCriterion
    from controllable_xgating_amd.driver import decode_sequence, eval_split
    cfg = dict(CFG["tiny"]); cfg["B"] = 3
    d = pg.make_dims(**cfg)
    model = make_model(d, train=True, p_drop=p_drop)
    itow = {i: "w%d" % i for i in range(1, d.V)}
    batches = []
    for seed in (0, 1):
        x = to_dev(pg.make_inputs(d, seed=seed, ragged=True))
        x["image_ids"] = ["vid%d_%d" % (seed, k) for k in range(d.B)]
        batches.append(x)
    loss, preds, stats = eval_split(model, LanguageModelCriterion(), ClassiferCriterion(), batches, itow,
                                    {"beam_size": beam, "weight_class": WEIGHT_CLASS, "language_eval": 1},
                                    gts_of={i: [i] for b in batches for i in b["image_ids"]},
                                    scorer=lambda caps, gts: {"n": len(caps), "same": len(caps) == len(gts)})
    assert model.training and stats == {"n": 2 * d.B, "same": True}
    assert [p["image_id"] for p in preds] == batches[0]["image_ids"] + batches[1]["image_ids"]
    P = xo.to_torch_params(pg.make_params(d))
    want_loss, want_sents = 0.0, []
    for seed in (0, 1):
        xi = xo.to_torch_inputs(pg.make_inputs(d, seed=seed, ragged=True))
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"], xi["seq_mask"],
                                     train=False, p=0.0, seed=0, running=xo.new_running(d))
        want_loss += float(xo.lm_criterion(logp, xi["seq"], xi["seq_mask"])) + \
            WEIGHT_CLASS * float(xo.cls_criterion(cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"]))
        if beam == 1:
            seq, _ = xo.sample(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], d.L, mode="greedy",
                               train=False, running=xo.new_running(d))
            want_sents += decode_sequence(itow, seq)
    assert abs(loss - want_loss / 2) < 2e-5 * max(1.0, abs(want_loss))
    if beam == 1:
        assert [p["caption"] for p in preds] == want_sents
    else:       # batch 0 is the beam-search golden's input (seed 0, not ragged there: compare only when masks agree)
        g = load_golden("beam_tiny.npz")
        x0 = to_dev(pg.make_inputs(d, seed=0))
        x0["image_ids"] = batches[0]["image_ids"]
        _, p0, _ = eval_split(model, LanguageModelCriterion(), ClassiferCriterion(), [x0], itow, {"beam_size": int(g["beam_size"])})
        assert [p["caption"] for p in p0] == decode_sequence(itow, g["seq"])


def test_three_iteration_xe_trajectory_vs_oracle_loop():
    """zero_grad -> forward -> criteria -> backward -> clamp +-0.1 -> Adam, three times (starttrain.py:123-137)."""
    import argparse
    from controllable_xgating_amd.driver import Trainer
    d = pg.make_dims(**CFG["mid"])
    model = make_model(d)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    opt = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, weight_class=WEIGHT_CLASS,
                             learning_rate_decay_start=-1, scheduled_sampling_start=-1, self_critical_after=-1)
    tr = Trainer(model, opt)
    tr.start_epoch(0)
    batch = dict(feat1=x["feats_rgb"], feat2=x["feats_opfl"], feat_mask=x["feat_mask"], pos_feat=x["pos_feats"], cap=x["seq"],
                 cap_mask=x["seq_mask"], cap_classes=x["cap_classes"], class_mask=x["class_mask"])
    hip_losses = [tr.train_batch(batch)["loss"].item() for _ in range(3)]
    # oracle loop
    P = xo.to_torch_params(pg.make_params(d), requires_grad=True)
    xi = xo.to_torch_inputs(pg.make_inputs(d, seed=0, ragged=True))
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    v = {k: torch.zeros_like(v_) for k, v_ in P.items()}
    running = xo.new_running(d)
    ora_losses = []
    for step in (1, 2, 3):
        for t in P.values():
            t.grad = None
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"],
                                     xi["seq_mask"], train=True, running=running)
        loss = xo.lm_criterion(logp, xi["seq"], xi["seq_mask"]) + WEIGHT_CLASS * xo.cls_criterion(
            cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"])
        loss.backward()
        ora_losses.append(loss.item())
        with torch.no_grad():
            for k in P:
                g = P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])
                pn, m[k], v[k] = xo.adam_step(P[k].detach(), g.clamp(-0.1, 0.1), m[k], v[k], step, 4e-4)
                P[k].copy_(pn)
    np.testing.assert_allclose(hip_losses, ora_losses, atol=2e-4)
    assert hip_losses[2] < hip_losses[0]
    for name, prm in model.named_parameters():
        # parameters whose true gradient is exactly zero (Linear bias in front of train-mode BatchNorm; a2w.bias, which
        # cancels in the softmax) see only round-off noise, and Adam turns noise of any size into +-lr steps: skip them
        if name.endswith("visual_emb_rgb.0.bias") or name.endswith("visual_emb_opfl.0.bias") or name == "lstmcore.a2w.bias":
            continue
        np.testing.assert_allclose(prm.detach().cpu().numpy(), P[name].detach().numpy(), atol=2e-5, err_msg=name)


def test_scst_iteration_and_checkpoint_roundtrip(tmp_path):
    import argparse
    from controllable_xgating_amd.driver import Trainer
    d = pg.make_dims(**CFG["mid"])
    model = make_model(d, P=pg.make_params(d, logit_gain=1.0))
    x = to_dev(pg.make_inputs(d, seed=0))
    opt = argparse.Namespace(learning_rate=4e-4, weight_decay=0.0, grad_clip=0.1, weight_class=0.0,
                             learning_rate_decay_start=-1, scheduled_sampling_start=-1, self_critical_after=0, patience=2)
    rew = pg.uniform("reward2", (2 * d.B,), 3, 0.0, 1.0)
    tr = Trainer(model, opt, reward_scorer=lambda gen, greedy: rew)          # CIDEr stubbed (BASELINE.json config 3)
    tr.start_epoch(0)
    assert tr.sc_flag
    batch = dict(feat1=x["feats_rgb"], feat2=x["feats_opfl"], feat_mask=x["feat_mask"], pos_feat=x["pos_feats"])
    before = model.flat_parameters().clone()
    info = tr.train_batch(batch)
    assert np.isfinite(info["loss"].item())
    assert abs(info["avg_reward"] - float(np.mean(rew[:d.B] - rew[d.B:]))) < 1e-6        # np.mean(reward[:, 0]), starttrain.py:145
    assert not torch.equal(before, model.flat_parameters())
    assert tr.update_best(str(tmp_path), 0.5) is False
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    tr.train_batch(batch)
    Trainer.resume(model, str(tmp_path))
    for k, v in model.state_dict().items():
        assert torch.equal(v, saved[k]), k
    assert tr.update_best(str(tmp_path), 0.4) is False and tr.update_best(str(tmp_path), 0.3) is True   # patience 2


# ---------------------------------------------------------------- scheduled sampling
def test_scheduled_sampling_vs_oracle():
    """ss_prob = 0.5 with supplied uniforms: same replaced tokens, loss and gradients as the oracle (whose
    scheduled-sampling semantics are pinned by the reference replay golden ss_tiny.npz)."""
    from controllable_xgating_amd import LanguageModelCriterion
    d = pg.make_dims(**CFG["mid"])
    T = d.L + 1
    u_sel = pg.uniform("ss.sel", (T, d.B), 31)
    u_tok = pg.uniform("ss.tok", (T, d.B), 32)
    P = xo.to_torch_params(pg.make_params(d), requires_grad=True)
    xi = xo.to_torch_inputs(pg.make_inputs(d, seed=0, ragged=True))
    its = []
    logp_o, cat_o, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"],
                                     xi["seq_mask"], train=True, running=xo.new_running(d), ss_prob=0.5, u_sel=u_sel,
                                     u_tok=u_tok, it_trace=its)
    loss_o = xo.lm_criterion(logp_o, xi["seq"], xi["seq_mask"])
    loss_o.backward()
    its = torch.stack(its).numpy()
    assert (its != xi["seq"].numpy().T).sum() > 10                   # tokens really were replaced
    model = make_model(d)
    model.ss_prob = 0.5
    model.ss_uniforms = (torch.from_numpy(u_sel).cuda(), torch.from_numpy(u_tok).cuda())
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    loss = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_o.item()) < 1e-4, (loss.item(), loss_o.item())
    np.testing.assert_allclose(logp.detach().cpu().numpy(), logp_o.detach().numpy(), atol=3e-4)
    np.testing.assert_allclose(cat.detach().cpu().numpy(), cat_o.detach().numpy(), atol=1e-4)
    assert_grads_close(model, oracle_grads(P))
    # eval mode ignores ss_prob (SAModel.py:89: `if self.training and ...`)
    model.eval()
    with torch.no_grad():
        l_eval, _ = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    model.ss_prob = 0.0
    with torch.no_grad():
        l_ref, _ = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    assert torch.equal(l_eval, l_ref)


# ---------------------------------------------------------------- bf16 matrix-core modes (BASELINE.json configs[4])
@pytest.mark.parametrize("ta,tb", gs.LAYOUT_CASES)
@pytest.mark.parametrize("M,N,K", gs.BF16_OPERANDS)
def test_gemm_bf16_operands_in_memory(M, N, K, ta, tb):
    """Both operands bf16 in memory (xg_gemm_bf16_operands; round 5: tiles by LDS-DMA, xg_gemm_g16.hip, where the shape
    qualifies -- ragged M / N edges, a K tail next to an m-contiguous operand, deep reductions split across workgroups; the
    register-staged kernel elsewhere).  The operands ARE the bf16 values, so the product is checked element by element against
    fp64 of the same values at fp32-accumulation tolerance -- a misplaced fragment or a wrong swizzle cannot hide in bf16
    round-off."""
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g = torch.Generator().manual_seed(11 * M + 5 * N + K + ta * 2 + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=g).bfloat16(); Bm = torch.randn((N, K) if tb else (K, N), generator=g).bfloat16()
    bias = torch.randn(N, generator=g); C0 = torch.randn(M, N, generator=g)
    ref = (A.t() if ta else A).double() @ (Bm.t() if tb else Bm).double() + bias.double()
    A16, B16, bd = A.cuda(), Bm.cuda(), bias.cuda()
    Af, Bf = A16.float(), B16.float()
    for relu, acc in ((0, 0), (1, 0), (0, 1)):
        Cd = C0.clone().cuda()
        assert L.xg_gemm_bf16_operands(None, ta, tb, M, N, K, nv.ptr(Af), nv.ptr(A16), A.shape[1], nv.ptr(Bf), nv.ptr(B16), Bm.shape[1],
                                       nv.ptr(Cd), N, nv.ptr(bd), relu, acc) == 0
        want = ref + (C0.double() if acc else 0)
        if relu:
            want = want.clamp(min=0)
        err = float((Cd.cpu().double() - want).abs().max())
        assert err <= (2e-6 * np.sqrt(K) * 4 + 1e-6) * max(1.0, float(want.abs().max())), (relu, acc, err)


@pytest.mark.parametrize("ta,tb", gs.LAYOUT_CASES)
@pytest.mark.parametrize("M,N,K", gs.BF16_MODES)
def test_gemm_bf16_modes(M, N, K, ta, tb):
    """mode 3 (split-bf16, 6 MFMAs) must be fp32-class; mode 1 (bf16 operands) within bf16 round-off."""
    from controllable_xgating_amd import _native as nv
    L = nv.lib()
    g = torch.Generator().manual_seed(M + N + K + ta * 2 + tb)
    A = torch.randn((K, M) if ta else (M, K), generator=g); Bm = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g); C0 = torch.randn(M, N, generator=g)
    ref = (A.t() if ta else A).double() @ (Bm.t() if tb else Bm).double() + bias.double()
    Ad, Bd, bd = A.cuda(), Bm.cuda(), bias.cuda()
    for mode, tol in ((3, 4e-6), (1, 2e-2)):
        for relu, acc in ((0, 0), (1, 0), (0, 1)):
            Cd = C0.clone().cuda()
            assert L.xg_gemm_mode(None, mode, ta, tb, M, N, K, nv.ptr(Ad), A.shape[1], nv.ptr(Bd), Bm.shape[1], nv.ptr(Cd), N,
                                  nv.ptr(bd), relu, acc) == 0
            want = ref + (C0.double() if acc else 0)
            if relu:
                want = want.clamp(min=0)
            err = float((Cd.cpu().double() - want).abs().max()) / float(want.abs().max())
            assert err < tol, (mode, relu, acc, err)


def test_config5_bf16_within_1e2_of_fp32_reference_golden():
    """BASELINE.json configs[4]: hidden 1024, 40 frames, vocab 20k with the large products on the bf16 matrix cores;
    loss within 1e-2 of the reference's fp32 result (north_star tolerance for the bf16 config)."""
    from controllable_xgating_amd import LanguageModelCriterion, SAModel, make_opt
    g = load_golden("xe_c5.npz")
    d = pg.make_dims(**CFG["c5"])
    model = SAModel(make_opt(d, precision="bf16"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in pg.make_params(d).items()}, strict=False)
    model = model.cuda(); model.train()
    x = to_dev(pg.make_inputs(d, seed=0))
    from controllable_xgating_amd import ClassiferCriterion
    logp, cat = model(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    loss = LanguageModelCriterion()(logp, x["seq"], x["seq_mask"])
    total = loss + WEIGHT_CLASS * ClassiferCriterion()(cat, x["cap_classes"], x["seq_mask"], x["class_mask"])
    total.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(g["loss_xe"])) < 1e-2, (loss.item(), float(g["loss_xe"]))
    assert abs(total.item() - float(g["loss"])) < 1e-2
    for name, prm in model.named_parameters():
        gn = float(prm.grad.double().norm())
        ref_n = float(g["gnorm/" + name])
        assert abs(gn - ref_n) <= 5e-2 * ref_n + 1e-5, (name, gn, ref_n)
    # and the split-bf16 mode is fp32-class on the same config
    model3 = SAModel(make_opt(d, precision="bf16x3"))
    model3.load_state_dict({k: torch.from_numpy(v) for k, v in pg.make_params(d).items()}, strict=False)
    model3 = model3.cuda(); model3.train()
    logp3, _ = model3(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    loss3 = LanguageModelCriterion()(logp3, x["seq"], x["seq_mask"])
    assert abs(loss3.item() - float(g["loss_xe"])) < 1e-4, (loss3.item(), float(g["loss_xe"]))


def test_scst_rollout_modes_equal_the_sequential_reference_order():
    """scst_rollouts: "batched" (one 2m-row pass, xg_rollout_pair + xg_rollout_compact) and "streams" (greedy baseline on
    a side stream) == the sequential reference order: same tokens, same log-probs, same BatchNorm running statistics after
    the two updates, and the same policy-gradient parameter gradients."""
    from controllable_xgating_amd import RewardCriterion
    from controllable_xgating_amd.driver import scst_rollouts
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0))
    u = torch.from_numpy(pg.uniform("uni2", (d.L + 1, d.B), 78)).cuda()
    reward = torch.from_numpy(pg.uniform("rew", (d.B, 1), 5)).cuda() - 0.5
    outs = []
    for mode in ("sequential", "streams", "batched"):
        model = make_model(d, P=Pn, train=True)
        gen, slp, greedy = scst_rollouts(model, x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], mode=mode, uniforms=u)
        loss = RewardCriterion()(slp, gen, reward.expand(-1, gen.shape[1]))
        loss.backward()
        torch.cuda.synchronize()
        bn = model.two_spatial_encoder.visual_emb_rgb[1]
        grads = {n: q.grad.detach().cpu().numpy().copy() for n, q in model.named_parameters()}
        outs.append((gen.cpu().numpy(), slp.detach().cpu().numpy(), greedy.cpu().numpy(), bn.running_mean.cpu().numpy(),
                     bn.running_var.cpu().numpy(), int(bn.num_batches_tracked), grads))
    a = outs[0]
    assert a[0].shape[1] > 0 and a[2].shape[1] > 0
    for b in outs[1:]:
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        np.testing.assert_allclose(a[1], b[1], atol=2e-6)
        np.testing.assert_allclose(a[3], b[3], atol=1e-6)
        np.testing.assert_allclose(a[4], b[4], atol=1e-6)
        assert a[5] == b[5] == 2
        for n in a[6]:       # same policy as assert_grads_close (the batched pass runs other GEMM tilings: fp32 round-off)
            err, scale = float(np.abs(a[6][n] - b[6][n]).max()), float(np.abs(a[6][n]).max())
            assert err <= 2e-6 + 2e-3 * scale, (n, err, scale)


def test_scst_paired_rollout_bf16_mirrors_survive_the_compaction():
    """precision='bf16' (gemm_mode 1): the large products read bf16 mirrors of their operands in the workspace.  The paired
    SCST rollout runs in a 2m-row workspace and its sampled half is COMPACTED into an m-row workspace for the backward
    (xg_rollout_compact copies no mirrors: xg_rollout_bwd converts the encoder-side operands again).  Gradients of the paired
    path == gradients of the plain m-row rollout with the same draws, at sizes where every product takes the bf16 kernels
    (B K >= 256, T B >= 256, all pitches multiples of 8)."""
    from controllable_xgating_amd import RewardCriterion, SAModel, make_opt
    from controllable_xgating_amd.driver import scst_rollouts
    d = pg.make_dims(B=16, K=20, R=256, A=384, E=64, V=2000, C=14, L=20, F1=96, F2=64)
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0))
    u = torch.from_numpy(pg.uniform("uni_bf", (d.L + 1, d.B), 13)).cuda()
    reward = torch.from_numpy(pg.uniform("rew_bf", (d.B, 1), 5)).cuda() - 0.5
    outs = []
    for mode in ("sequential", "batched"):
        model = SAModel(make_opt(d, precision="bf16"))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in Pn.items()}, strict=False)
        model = model.cuda(); model.train()
        gen, slp, greedy = scst_rollouts(model, x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], mode=mode, uniforms=u)
        loss = RewardCriterion()(slp, gen, reward.expand(-1, gen.shape[1]))
        loss.backward()
        torch.cuda.synchronize()
        outs.append((gen.cpu().numpy(), float(loss.item()), {n: q.grad.detach().cpu().numpy().copy() for n, q in model.named_parameters()}))
    a, b = outs
    assert a[0].shape == b[0].shape and (a[0] != b[0]).mean() < 0.02          # (bf16 logits: a rare near-tie may flip a draw)
    if np.array_equal(a[0], b[0]):
        assert abs(a[1] - b[1]) < 2e-3 * max(1.0, abs(a[1]))
        for n in a[2]:
            if n in ZERO_GRAD_PARAMS:
                continue
            err, scale = float(np.abs(a[2][n] - b[2][n]).max()), float(np.abs(a[2][n]).max())
            assert err <= 1e-6 + 3e-2 * scale, (n, err, scale)


def test_gradsync_overlapped_allreduce_single_rank():
    """train.GradSync: the two-part all-reduce started from the library's grad-ready event (XgRun.grad_event) leaves
    the same gradients as the plain path (single-rank RCCL group: the collective is the identity, the event / stream /
    slicing mechanics are what is exercised), for the fused XE backward and the rollout backward."""
    import torch.distributed as dist
    from controllable_xgating_amd import RewardCriterion
    from controllable_xgating_amd import train as tr
    created = False
    if not dist.is_initialized():
        import socket
        with socket.socket() as sk:                     # a free port on the loopback interface
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
        created = True
    old_force = tr._FORCE
    tr._FORCE = True
    try:
        d = pg.make_dims(**CFG["mid"])
        Pn = pg.make_params(d, logit_gain=1.0)
        x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
        u = torch.from_numpy(pg.uniform("uni2", (d.L + 1, d.B), 78)).cuda()
        res = []
        for use_sync in (False, True):
            model = make_model(d, P=Pn, train=True)
            sync = tr.GradSync(model) if use_sync else None
            out = []
            for kind in ("xe", "rollout"):
                model.flat_grads().zero_()
                if kind == "xe":
                    loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
                else:
                    gen, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                            {"sample_max": 0, "uniforms": u})
                    loss = RewardCriterion()(slp, gen, torch.full_like(slp, 0.3))
                if sync is not None:
                    sync.arm()
                loss.backward()
                tr.allreduce_gradients(model)
                torch.cuda.synchronize()
                assert sync is None or not sync.armed
                out.append(model.flat_grads().detach().cpu().numpy().copy())
            res.append(out)
        for a, b in zip(res[0], res[1]):
            assert np.abs(a).max() > 0
            np.testing.assert_allclose(a, b, atol=2e-6 + 2e-3 * 0, rtol=2e-3)
    finally:
        tr._FORCE = old_force
        if created:
            dist.destroy_process_group()


def test_data_parallel_update_paths_agree_single_rank():
    """Three training iterations on a one-rank RCCL group (the collective is the identity; streams, events, segment slicing
    and the optimizer hand-off are what runs): (a) plain all-reduce + stream-ordered ClipAdam, (b) plain all-reduce with an
    ARMED overlapping ClipAdam(fused_zero) -- allreduce_gradients must disarm it, its segment updates would otherwise run
    behind events recorded before the collective --, (c) GradSync.finish with the armed overlapping optimizer (the default
    of driver.Trainer / bench.py: segment updates behind each bucket).  Same parameters and Adam moments after 3 steps."""
    import torch.distributed as dist
    from controllable_xgating_amd import train as tr
    created = False
    if not dist.is_initialized():
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
        created = True
    old_force = tr._FORCE
    tr._FORCE = True
    try:
        d = pg.make_dims(**CFG["mid"])
        Pn = pg.make_params(d)
        x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
        outs = {}
        for mode in ("plain", "plain+overlap", "gradsync+overlap"):
            model = make_model(d, P=Pn, train=True)
            over = mode != "plain"
            opt = tr.ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=over, fused_zero=over)
            sync = tr.GradSync(model) if mode.startswith("gradsync") else None
            for _ in range(3):
                opt.zero_grad()
                loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
                if sync is not None:
                    sync.arm()
                opt.arm()
                loss.backward()
                tr.allreduce_gradients(model)
                if mode == "plain+overlap":
                    assert not opt._armed and model._grad_event is None      # the plain collective disarmed the overlap
                opt.step()
            torch.cuda.synchronize()
            assert opt.step_count == 3
            if over:                                                        # fused_zero left the gradient buffer at zero
                assert float(model.flat_grads().abs().max()) == 0.0
            outs[mode] = (model.flat_parameters().detach().cpu().numpy().copy(), opt.exp_avg.cpu().numpy().copy(),
                          opt.exp_avg_sq.cpu().numpy().copy(), float(loss.item()))
        ref = outs["plain"]
        assert np.abs(ref[1]).max() > 0
        for mode in ("plain+overlap", "gradsync+overlap"):
            got = outs[mode]
            assert abs(got[3] - ref[3]) < 1e-5, (mode, got[3], ref[3])
            np.testing.assert_allclose(got[1], ref[1], atol=1e-6 + 2e-3 * np.abs(ref[1]).max(), err_msg=mode)
            np.testing.assert_allclose(got[2], ref[2], atol=1e-9 + 2e-3 * np.abs(ref[2]).max(), err_msg=mode)
            # Adam normalises: elements with round-off-level gradients may step differently (<= 3 lr after three steps)
            disp = np.abs(got[0] - ref[0])
            assert disp.max() <= 3.1 * 4e-4 and (disp > 4e-5).mean() <= 0.02, (mode, float(disp.max()), float((disp > 4e-5).mean()))
    finally:
        tr._FORCE = old_force
        if created:
            dist.destroy_process_group()


def test_graphed_xe_step_equals_the_eager_loop():
    """train.GraphedXEStep: the whole XE training iteration (zero_grad, fused forward + loss, backward, clamp + Adam with its
    step-dependent scalars in device memory, weight re-pack) captured once as a HIP graph; four replays give the losses,
    parameters, Adam moments and BatchNorm statistics of four eager iterations, and building the graph leaves the model
    untouched.  (The eager loop itself follows the reference trajectory: test_three_iteration_trajectory_vs_reference_adam_golden.)"""
    from controllable_xgating_amd import train as tr
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    outs = {}
    for mode in ("eager", "eager_dev", "graph"):
        model = make_model(d, P=Pn, train=True)
        opt = tr.ClipAdam(model, lr=4e-4, grad_clip=0.1, overlap=True, fused_zero=True, device_state=mode != "eager")
        losses = []
        if mode == "graph":
            p0 = model.flat_parameters().clone()
            step = tr.GraphedXEStep(model, opt, x, weight_class=WEIGHT_CLASS)
            assert torch.equal(p0, model.flat_parameters()) and opt.step_count == 0      # construction has no side effects
            for _ in range(4):
                losses.append(float(step().item()))
        else:
            for _ in range(4):
                opt.zero_grad()
                loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"],
                                     x["cap_classes"], x["class_mask"], WEIGHT_CLASS)
                opt.arm(); loss.backward(); opt.step()
                losses.append(float(loss.item()))
        torch.cuda.synchronize()
        bn = model.two_spatial_encoder.visual_emb_rgb[1]
        outs[mode] = (losses, model.flat_parameters().detach().cpu().numpy().copy(), opt.exp_avg.cpu().numpy().copy(),
                      opt.exp_avg_sq.cpu().numpy().copy(), bn.running_mean.cpu().numpy().copy(), int(bn.num_batches_tracked), opt.step_count)
    ref = outs["eager"]
    assert ref[0][3] < ref[0][0]
    for mode in ("eager_dev", "graph"):
        got = outs[mode]
        np.testing.assert_allclose(got[0], ref[0], atol=2e-5, err_msg=mode)
        np.testing.assert_allclose(got[2], ref[2], atol=1e-6 + 2e-3 * np.abs(ref[2]).max(), err_msg=mode)
        np.testing.assert_allclose(got[3], ref[3], atol=1e-9 + 2e-3 * np.abs(ref[3]).max(), err_msg=mode)
        disp = np.abs(got[1] - ref[1])
        assert disp.max() <= 4.1 * 4e-4 and (disp > 4e-5).mean() <= 0.02, (mode, float(disp.max()), float((disp > 4e-5).mean()))
        np.testing.assert_allclose(got[4], ref[4], atol=1e-4, err_msg=mode)      # (a function of the updated embedding weights)
        assert got[5] == ref[5] == 4 and got[6] == 4, (mode, got[5], got[6])


def test_packed_weights_are_ordered_across_streams():
    """The packed shadow of the recurrent weights is rewritten on the stream of the first call after a parameter update; a
    call on ANOTHER stream right behind it must wait for that pack (model._packed_ptr records an event): a rollout issued on
    a side stream immediately after an optimizer step gives the same tokens / log-probs as the same rollout on the main stream."""
    from controllable_xgating_amd import train as tr
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0))
    u = torch.from_numpy(pg.uniform("uni_pk", (d.L + 1, d.B), 7)).cuda()
    outs = []
    for side_first in (False, True):
        model = make_model(d, P=Pn, train=True)
        opt = tr.ClipAdam(model, lr=1e-2, grad_clip=0.1)
        for it in range(3):
            opt.zero_grad()
            loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
            loss.backward()
            opt.step()                                           # -> mark_params_changed: the next call re-packs
            main = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            with torch.no_grad():
                if side_first:                                   # pack happens on `side`; the main-stream call must wait for it
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                     {"sample_max": 1, "async": True, "bn_update": False})
                seq, slp, n = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                           {"sample_max": 0, "uniforms": u, "async": True, "bn_update": False})
                main.wait_stream(side)
        torch.cuda.synchronize()
        outs.append((seq.cpu().numpy(), slp.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    # (a few ulp: the two halves of a video's attention context meet in fp32 atomics, whose order follows the scheduling)
    np.testing.assert_allclose(outs[0][1], outs[1][1], atol=5e-6)


def test_reward_criterion_scalar_and_per_position_rewards():
    """RewardCriterion broadcasts like the reference's ``input * reward`` (SAModel.py:262): a 0-d scalar, one value per video
    (m,) / (m, 1), one row (1, L), and the full (m, L) matrix."""
    from controllable_xgating_amd import RewardCriterion
    g = torch.Generator().manual_seed(3)
    m, L = 6, 9
    slp = (-torch.rand(m, L, generator=g)).cuda().requires_grad_(True)
    seq = torch.randint(0, 4, (m, L), generator=g).cuda()
    crit = RewardCriterion()

    def ref(reward):
        mask = torch.cat([torch.ones(m, 1, device="cuda"), (seq[:, :-1] > 0).float()], 1)
        return -(slp.detach() * reward * mask).sum() / mask.sum()
    row = torch.rand(1, L, generator=g).cuda()
    per_video = torch.rand(m, generator=g).cuda()
    for reward, full in ((torch.tensor(0.7), torch.full((m, L), 0.7, device="cuda")), (per_video, per_video[:, None].expand(m, L)),
                         (row, row.expand(m, L)), (0.25, torch.full((m, L), 0.25, device="cuda"))):
        loss = crit(slp, seq, reward)
        assert abs(loss.item() - ref(full).item()) < 1e-6
        loss.backward()
    # a 1-D reward of length L != m is one value per POSITION; the flattened (m*L,) vector is the reference's own view(-1) form
    per_pos = torch.rand(L, generator=g).cuda()
    assert abs(crit(slp, seq, per_pos).item() - ref(per_pos[None, :].expand(m, L)).item()) < 1e-6
    full = torch.rand(m, L, generator=g).cuda()
    assert abs(crit(slp, seq, full.reshape(-1)).item() - ref(full).item()) < 1e-6
    # m == L: a 1-D reward of that length could mean either -- the reference never broadcasts (SAModel.py:260-261 flattens both
    # tensors), so the ambiguous form is rejected and the two explicit ones are accepted
    from controllable_xgating_amd._native import XgError
    sq = slp.detach()[:, :m].contiguous().requires_grad_(True)
    seq_sq, pp = seq[:, :m].contiguous(), per_pos[:m].contiguous()
    with pytest.raises(XgError):
        crit(sq, seq_sq, pp)
    mask = torch.cat([torch.ones(m, 1, device="cuda"), (seq_sq[:, :-1] > 0).float()], 1)
    want_pos = -(sq.detach() * pp[None, :] * mask).sum() / mask.sum()
    want_vid = -(sq.detach() * pp[:, None] * mask).sum() / mask.sum()
    assert abs(crit(sq, seq_sq, pp[None, :]).item() - want_pos.item()) < 1e-6
    assert abs(crit(sq, seq_sq, pp[:, None]).item() - want_vid.item()) < 1e-6


def test_repeated_iterations_are_reproducible_across_streams():
    """The forward / backward passes run on three HIP streams (main + two auxiliary ones).  A missing dependency between
    them would show up as run-to-run differences far above the fp32-atomic summation noise: the same iteration five
    times (config-2-like proportions, both the fused XE path and the paired SCST path) must give the same loss and
    gradients every time."""
    from controllable_xgating_amd import RewardCriterion
    d = pg.make_dims(B=32, K=13, R=128, A=192, E=68, V=1200, C=14, L=11, F1=96, F2=64)
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=3, ragged=True))
    u = torch.from_numpy(pg.uniform("uni3", (d.L + 1, d.B), 11)).cuda()
    model = make_model(d, P=Pn, train=True)
    ref = {}
    for rep in range(5):
        for kind in ("xe", "pair"):
            model.flat_grads().zero_()
            if kind == "xe":
                loss = model.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"],
                                     x["cap_classes"], x["class_mask"], WEIGHT_CLASS)
            else:
                gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"],
                                                        {"uniforms": u})
                loss = RewardCriterion()(slp, gen, torch.full_like(slp, 0.25))
            loss.backward()
            torch.cuda.synchronize()
            g = model.flat_grads().detach().cpu().numpy().copy()
            lv = float(loss.item())
            if rep == 0:
                ref[kind] = (lv, g)
                assert np.isfinite(g).all() and np.abs(g).max() > 0
            else:
                assert abs(lv - ref[kind][0]) <= 1e-6 * max(1.0, abs(ref[kind][0])), (kind, rep, lv, ref[kind][0])
                err = np.abs(g - ref[kind][1]).max()
                assert err <= 1e-5 * np.abs(ref[kind][1]).max() + 1e-8, (kind, rep, float(err))


def test_single_stream_path_equals_multi_stream_path():
    """XgRun.aux = NULL (everything on the caller's stream: no side streams, no background products, no zero block on a side
    stream) against the default three-stream schedule: same loss, same gradients after an XE backward and after a rollout
    backward on top of it."""
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    args = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    u = torch.from_numpy(pg.uniform("uni_ss", (d.L + 1, d.B), 5)).cuda()
    outs = []
    for single in (False, True):
        m = make_model(d)
        if single:
            m._aux_handle = lambda: None
        m.flat_grads().zero_()
        loss = m.xe_loss(*args)
        loss.backward()
        torch.cuda.synchronize()
        g_xe = m.flat_grads().detach().cpu().numpy().copy()
        gen, slp, greedy, n = m.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"uniforms": u})
        slp.sum().backward()
        torch.cuda.synchronize()
        outs.append((float(loss.detach()), g_xe, m.flat_grads().detach().cpu().numpy().copy(), gen.cpu().numpy()))
    (l0, a0, b0, s0), (l1, a1, b1, s1) = outs
    assert abs(l0 - l1) < 5e-6 * max(1.0, abs(l0))
    assert np.array_equal(s0, s1)
    assert np.abs(a0 - a1).max() <= 1e-5 * np.abs(a0).max() + 1e-8
    assert np.abs(b0 - b1).max() <= 1e-5 * np.abs(b0).max() + 1e-8


def _fuzz_dims(i):
    """Seeded random extents that hit the kernel-selection edges: R % 8 / % 4 (skinny vs generic cells, fused LSTM
    backward), A % 4 and A > 1024 (attention variants), K > 32 (16 V rows per thread) and K > 64 (serial softmax),
    E % 4 (vector vs scalar skinny loads), odd V, B = 1."""
    rng = np.random.RandomState(1000 + i)
    R = int(rng.choice([8, 16, 24, 40, 64, 72, 12, 20, 128]))
    A = int(rng.choice([8, 36, 64, 100, 256, 260, 1280]))
    K = int(rng.choice([1, 2, 7, 26, 33, 40, 70]))
    E = int(rng.choice([4, 10, 36, 68]))
    return dict(B=int(rng.choice([1, 2, 5, 9, 33])), K=K, R=R, A=A, E=E, V=int(rng.choice([5, 37, 64, 301])),
                C=int(rng.choice([2, 14])), L=int(rng.choice([1, 3, 6, 9])), F1=int(rng.choice([4, 20, 48])),
                F2=int(rng.choice([4, 12, 40])), H=128)


@pytest.mark.parametrize("i", range(24))
def test_fuzzed_extents_xe_and_greedy_vs_oracle(i):
    cfg = _fuzz_dims(i)
    d = pg.make_dims(**cfg)
    ragged = bool(i % 2) and d.L >= 2 and d.K >= 2
    drop, seed = (0.3, 4242 + i) if i % 3 == 0 else (0.0, None)     # every third case with dropout (hash masks)
    P, lo, co, lxe_o, lcls_o, running = run_oracle_xe(d, ragged, p=drop, seed=seed or 0)
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, ragged, p=drop, seed=seed)
    assert abs(lxe_h - lxe_o) < 1e-4, (cfg, lxe_h, lxe_o)
    assert abs(lcls_h - lcls_o) < 1e-4, cfg
    np.testing.assert_allclose(lh, lo, atol=3e-4, rtol=0, err_msg=str(cfg))
    assert_grads_close(model, oracle_grads(P), skip=ZERO_GRAD_PARAMS)
    # greedy rollout: token for token wherever the oracle's top-2 margin is not at round-off level
    x = pg.make_inputs(d, seed=0, ragged=ragged)
    Pt = xo.to_torch_params(pg.make_params(d))
    xt = xo.to_torch_inputs(x)
    with torch.no_grad():
        seq_o, slp_o, logps = xo.sample(Pt, xt["feats_rgb"], xt["feats_opfl"], xt["feat_mask"], xt["pos_feats"], d.L,
                                        mode="greedy", train=False, running=xo.new_running(d), return_logp=True)
    model = make_model(d, train=False)            # fresh BatchNorm running statistics, like the oracle's
    xd = to_dev(x)
    with torch.no_grad():
        seq_h, slp_h = model.sample(xd["feats_rgb"], xd["feats_opfl"], xd["feat_mask"], xd["pos_feats"], {"sample_max": 1})
    seq_o, seq_h = np.asarray(seq_o), seq_h.cpu().numpy()
    n = min(seq_o.shape[1], seq_h.shape[1])
    for b in range(d.B):
        for t in range(n):
            if seq_h[b, t] != seq_o[b, t]:
                top2 = np.sort(np.asarray(logps[t])[b])[-2:]
                assert top2[1] - top2[0] < 1e-3, (cfg, b, t, int(seq_h[b, t]), int(seq_o[b, t]), float(top2[1] - top2[0]))
                break                                   # the rows diverge after a (legitimate) near-tie
        else:
            if n:
                np.testing.assert_allclose(slp_h.cpu().numpy()[b, :n], np.asarray(slp_o)[b, :n], atol=2e-4, err_msg=str(cfg))


@pytest.mark.parametrize("cfg", [
    # vocabulary sizes that select each cross-entropy variant: register-resident rows of 2 / 5 / 8 16-byte pieces per
    # thread and the streaming kernel beyond 32768 (xg_heads.hip: xgk_xent_fwd), with the early / late row split
    dict(B=3, K=5, R=16, A=24, E=12, V=8192, C=4, L=5, F1=8, F2=8, H=128),
    dict(B=3, K=5, R=16, A=24, E=12, V=24004, C=4, L=5, F1=8, F2=8, H=128),
    dict(B=2, K=4, R=16, A=24, E=12, V=33000, C=4, L=4, F1=8, F2=8, H=128),
    # more than 32 decoder steps: the attention backward's tail kernels leave their register-resident forms
    # (xg_attn.hip: attn_bwd_post_kernel<0>, attn_dV_kernel); the weight gradients of the late steps are enqueued under the loop
    dict(B=4, K=6, R=16, A=24, E=12, V=50, C=4, L=36, F1=8, F2=8, H=128),
    # 25..32 steps: the 32-step forms
    dict(B=4, K=6, R=16, A=24, E=12, V=50, C=4, L=27, F1=8, F2=8, H=128),
    # attention widths that select the 4- and 8-group forms of the half-CU forward attention (xg_attn.hip: attn_fwd_fast<.., HALF>,
    # used beside the background vocabulary product of the teacher-forced forward) and the matching backward forms
    dict(B=3, K=9, R=16, A=1024, E=12, V=64, C=4, L=6, F1=8, F2=8, H=128),
    dict(B=2, K=34, R=16, A=2048, E=12, V=64, C=4, L=6, F1=8, F2=8, H=128),
], ids=["V8192", "V24004", "V33000", "T37", "T28", "A1024", "A2048K34"])
def test_kernel_variant_edges_xe_vs_oracle(cfg):
    d = pg.make_dims(**cfg)
    P, lo, co, lxe_o, lcls_o, running = run_oracle_xe(d, True, p=0.0, seed=0)
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, True, p=0.0, seed=None)
    assert abs(lxe_h - lxe_o) < 1e-4, (cfg, lxe_h, lxe_o)
    np.testing.assert_allclose(lh, lo, atol=3e-4, rtol=0, err_msg=str(cfg))
    assert_grads_close(model, oracle_grads(P), skip=ZERO_GRAD_PARAMS)
    # the fused loss path (xg_xe_loss_fwd / _bwd: row-split cross-entropy) against the same oracle gradients
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    m2 = make_model(d, train=True)
    m2.flat_grads().zero_()
    loss = m2.xe_loss(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"],
                      x["cap_classes"], x["class_mask"], WEIGHT_CLASS)
    loss.backward()
    assert abs(float(loss.detach()) - (lxe_o + WEIGHT_CLASS * lcls_o)) < 1e-4, cfg
    assert_grads_close(m2, oracle_grads(P), skip=ZERO_GRAD_PARAMS)


# ---------------------------------------------------------------- round 2: fixtures that pin what round 1 left unpinned
def test_greedy_with_natural_eos_token_for_token_vs_reference(p_drop=0.0):
    """greedy_c1_eos.npz: 44 distinct words, rows finish at steps 3..13 (two never do), live top-2 margins >= 2.4e-3 in the
    reference itself -> EOS / `unfinished` / zeroing of finished rows (SAModel.py:200-215) checked against the reference."""
    from tests.util import EOS_CASE, eos_params
    g = load_golden("greedy_c1_eos.npz")
    d = pg.make_dims(**CFG["c1"])
    model = make_model(d, P=eos_params(d), train=False, p_drop=p_drop)
    x = to_dev(pg.make_inputs(d, seed=EOS_CASE["input_seed"]))
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    seq, slp = seq.cpu().numpy(), slp.cpu().numpy()
    assert g["margin"][g["alive"]].min() >= 1e-3
    assert seq.shape == g["seq"].shape
    assert np.array_equal(seq, g["seq"]), np.argwhere(seq != g["seq"])
    np.testing.assert_allclose(slp, g["seqLogprobs"], atol=3e-4)


def test_raw_step_fwd_with_mask_and_alpha_vs_reference_golden():
    """xg_step_fwd driven RAW through ctypes with an xt_mask that holds row 2 and the alpha outlet: all of step_c1.npz
    (sub_modules.py:671-687; mask-hold :762,765), which get_logprobs_state (mask of ones, no alpha) cannot reach."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _stream, _ws_ptr
    g = load_golden("step_c1.npz")
    cfg = dict(CFG["c1"]); cfg["B"] = 4
    d = pg.make_dims(**cfg)
    model = make_model(d, train=True)
    B, K, R, E = d.B, d.K, d.R, d.E
    V = torch.from_numpy(pg.uniform("step.V", (B, K, R), 5, 0.0, 1.0)).cuda()
    pos = torch.from_numpy(pg.uniform("step.pos", (B, R), 5, -1.0, 1.0)).cuda()
    st0 = torch.cat([torch.from_numpy(pg.uniform(f"step.s{i}", (1, B, R), 5, -0.5, 0.5)) for i in range(4)], 0).cuda().contiguous()
    xt = torch.from_numpy(pg.uniform("step.xt", (B, E), 5, -0.1, 0.1)).cuda()
    with torch.no_grad():
        model.embed.weight[2:2 + B].copy_(xt)
    tok = torch.arange(2, 2 + B, device="cuda")
    mk = torch.tensor([1.0, 1.0, 0.0, 1.0], device="cuda")
    dd = model._dims(B, K, 1)
    ps, run = model._params_struct(), model._run(False)
    vproj = torch.empty(B, K, d.A, device="cuda")
    L = nv.lib()
    nv.check(L.xg_vproj(_stream(), C.byref(dd), C.byref(ps), nv.ptr(V), nv.ptr(vproj), C.byref(run)), "xg_vproj")
    ws = model._pool.shared(dd, V.device)
    wp, wn = _ws_ptr(ws)
    state = st0.clone()
    alpha = torch.zeros(B, K, device="cuda")
    logp = torch.empty(B, d.V, device="cuda")
    nv.check(L.xg_step_fwd(_stream(), C.byref(dd), C.byref(ps), nv.ptr(tok), nv.ptr(mk), nv.ptr(V), nv.ptr(vproj), nv.ptr(pos),
                           C.byref(run), 0, wp, wn, nv.ptr(state), nv.ptr(logp), nv.ptr(alpha)), "xg_step_fwd")
    torch.cuda.synchronize()
    s = state.cpu().numpy()
    np.testing.assert_allclose(s[0], g["h1"], atol=2e-5)
    np.testing.assert_allclose(s[1], g["c1"], atol=2e-5)
    np.testing.assert_allclose(s[2], g["h2"], atol=2e-5)
    np.testing.assert_allclose(s[3], g["c2"], atol=2e-5)
    np.testing.assert_allclose(s[2], g["out"], atol=2e-5)                  # output = h2' (:686)
    np.testing.assert_allclose(alpha.cpu().numpy(), g["alpha"], atol=2e-6)
    np.testing.assert_allclose(alpha.sum(1).cpu().numpy(), 1.0, atol=1e-5)
    assert np.array_equal(s[:, 2], st0.cpu().numpy()[:, 2])                # the held row keeps its state bit for bit
    # logp = log_softmax(logit(h2'))
    P = pg.make_params(d)
    want = torch.log_softmax(torch.from_numpy(g["out"]) @ torch.from_numpy(P["logit.weight"]).t() + torch.from_numpy(P["logit.bias"]), 1)
    np.testing.assert_allclose(logp.cpu().numpy(), want.numpy(), atol=3e-4)


@pytest.mark.parametrize("tag", ["tiny", "mid"])
def test_three_iteration_trajectory_vs_reference_adam_golden(tag):
    """driver.Trainer (zero_grad -> forward -> criteria -> backward -> xg_clip_adam) against the trajectory recorded from
    the REFERENCE model under torch.optim.Adam + the elementwise clamp (starttrain.py:76,123-137, myutils.py:79-85)."""
    import argparse
    from controllable_xgating_amd.driver import Trainer
    g = load_golden(f"traj_{tag}.npz")
    d = pg.make_dims(**CFG[tag])
    P0 = pg.make_params(d)
    model = make_model(d, P=P0)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    opt = argparse.Namespace(learning_rate=float(g["lr"]), weight_decay=0.0, grad_clip=float(g["grad_clip"]), weight_class=WEIGHT_CLASS,
                             learning_rate_decay_start=-1, scheduled_sampling_start=-1, self_critical_after=-1)
    tr = Trainer(model, opt)
    tr.start_epoch(0)
    batch = dict(feat1=x["feats_rgb"], feat2=x["feats_opfl"], feat_mask=x["feat_mask"], pos_feat=x["pos_feats"], cap=x["seq"],
                 cap_mask=x["seq_mask"], cap_classes=x["cap_classes"], class_mask=x["class_mask"])
    losses = [tr.train_batch(batch)["loss"].item() for _ in range(3)]
    np.testing.assert_allclose(losses, g["losses"], atol=1e-4)
    for name, prm in model.named_parameters():
        if name in ZERO_GRAD_PARAMS:
            continue
        idx = g["pidx/" + name]
        got = prm.detach().cpu().numpy().reshape(-1)[idx]
        # Adam normalises the gradient: an element whose gradient is at fp32 round-off level may step differently, so the
        # displacement (<= 3 lr) is compared at 10 % of lr for all but a handful of elements and the value at 3 lr
        np.testing.assert_allclose(got, g["psamp/" + name], atol=3.1 * float(g["lr"]), err_msg=name)
        disp_err = np.abs((got - P0[name].reshape(-1)[idx]) - g["dsamp/" + name])
        assert (disp_err > 4e-5).mean() <= 0.02, (name, float(disp_err.max()), float((disp_err > 4e-5).mean()))


def test_reward_criterion_hip_kernel_full_width_equals_trimmed_reference_form():
    """RewardCriterion (SAModel.py:259-267) as one HIP launch: (a) trimmed (m, n) inputs == the oracle's restatement, value
    and gradient; (b) full-width (m, L) inputs + the device-side early-exit width n == (a), with no host sync on n; (c) one
    reward per video (myutils.py:75-76) == the broadcast matrix."""
    from controllable_xgating_amd import RewardCriterion
    g = torch.Generator().manual_seed(11)
    m, L, n = 9, 14, 10
    seq = torch.randint(1, 50, (m, L), generator=g)
    for b in range(m):                                   # rows finish at different steps; nothing after column n-1
        end = 2 + (b * 3) % (n - 1)
        seq[b, end:] = 0
    seq[0, :n] = torch.randint(1, 50, (n,), generator=g)     # one row is alive through column n-1
    seq[:, n:] = 0
    slp = -torch.rand(m, L, generator=g) * 5
    rew_b = torch.randn(m, 1, generator=g)
    rew = rew_b.expand(-1, n).contiguous()
    crit = RewardCriterion()
    # (a) trimmed vs oracle
    s_o = slp[:, :n].clone().requires_grad_(True)
    lo = xo.reward_criterion(s_o, seq[:, :n], rew)
    lo.backward()
    s_a = slp[:, :n].clone().cuda().requires_grad_(True)
    la = crit(s_a, seq[:, :n].cuda(), rew.cuda())
    la.backward()
    assert abs(la.item() - lo.item()) < 1e-6
    np.testing.assert_allclose(s_a.grad.cpu().numpy(), s_o.grad.numpy(), atol=1e-7)
    # (b) full width + device n, (c) per-video reward
    s_b = slp.clone().cuda().requires_grad_(True)
    lb = crit(s_b, seq.cuda(), rew_b.cuda(), n=torch.tensor([n], dtype=torch.int32, device="cuda"))
    (2.0 * lb).backward()
    assert abs(lb.item() - lo.item()) < 1e-6
    np.testing.assert_allclose(s_b.grad.cpu().numpy()[:, :n], 2.0 * s_o.grad.numpy(), atol=1e-7)
    assert float(s_b.grad[:, n:].abs().max()) == 0.0


def test_sample_pair_leaves_reference_batchnorm_statistics():
    """SAModel.sample_pair called DIRECTLY (not through driver.scst_rollouts): running_mean / running_var /
    num_batches_tracked equal those after the reference's two sequential sample() calls (two momentum updates, unbiased
    variance of the N-row batch, not of the 2N repeated rows)."""
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0))
    u = torch.from_numpy(pg.uniform("uni2", (d.L + 1, d.B), 78)).cuda()
    ma = make_model(d, P=Pn, train=True)
    ma.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 0, "uniforms": u})
    with torch.no_grad():
        ma.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    mb = make_model(d, P=Pn, train=True)
    mb.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"uniforms": u})
    torch.cuda.synchronize()
    for mod in ("rgb", "opfl"):
        a = getattr(ma.two_spatial_encoder, f"visual_emb_{mod}")[1]
        b = getattr(mb.two_spatial_encoder, f"visual_emb_{mod}")[1]
        np.testing.assert_allclose(b.running_mean.cpu().numpy(), a.running_mean.cpu().numpy(), atol=1e-6)
        np.testing.assert_allclose(b.running_var.cpu().numpy(), a.running_var.cpu().numpy(), atol=1e-6)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 2


def test_sample_pair_with_train_mode_dropout_equals_two_independent_sample_calls():
    """Train mode with drop_prob_lm > 0 (the reference's default 0.5): the reference's two sample() calls (starttrain.py:131,
    myutils.py:45) draw INDEPENDENT dropout masks, in the encoder too.  sample_pair then runs as two rollouts with two seeds:
    tokens, log-probs, gradients and BatchNorm statistics equal those of sample(sample_max=0) followed by sample(sample_max=1)
    on a model in the same state -- and the greedy half really saw other masks than the sampled one."""
    from controllable_xgating_amd import RewardCriterion
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0))
    u = torch.from_numpy(pg.uniform("uni2", (d.L + 1, d.B), 78)).cuda()
    rew = torch.from_numpy(pg.uniform("rew.p", (d.B, 1), 5)).cuda() - 0.5
    ma = make_model(d, P=Pn, train=True, p_drop=0.5)
    mb = make_model(d, P=Pn, train=True, p_drop=0.5)
    ma._call = mb._call = 100                                # same seed sequence for both models
    gen_a, slp_a = ma.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 0, "uniforms": u})
    with torch.no_grad():
        greedy_a, _ = ma.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    RewardCriterion()(slp_a, gen_a, rew.expand(-1, gen_a.shape[1])).backward()
    gen_b, slp_b, greedy_b, n = mb.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"uniforms": u})
    nb = int(n[0])
    RewardCriterion()(slp_b[:, :nb], gen_b[:, :nb], rew.expand(-1, nb)).backward()
    torch.cuda.synchronize()
    na, ng = gen_a.shape[1], greedy_a.shape[1]
    assert nb == na and int(n[1]) == ng
    assert torch.equal(gen_a, gen_b[:, :na]) and torch.equal(greedy_a, greedy_b[:, :ng])
    np.testing.assert_allclose(slp_b[:, :na].detach().cpu().numpy(), slp_a.detach().cpu().numpy(), atol=1e-6)
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        np.testing.assert_allclose(pb.grad.cpu().numpy(), pa.grad.cpu().numpy(), atol=1e-6 + 1e-4 * float(pa.grad.abs().max()), err_msg=name)
    for mod in ("rgb", "opfl"):
        a = getattr(ma.two_spatial_encoder, f"visual_emb_{mod}")[1]
        b = getattr(mb.two_spatial_encoder, f"visual_emb_{mod}")[1]
        np.testing.assert_allclose(b.running_var.cpu().numpy(), a.running_var.cpu().numpy(), atol=1e-6)
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 2
    # independent masks: with ONE shared encoder realisation the greedy rollout would be the argmax path of the sampled rollout's
    # own encoder output; run it that way (same seed as the sampled call) and it must differ from what sample_pair returned
    mc = make_model(d, P=Pn, train=True, p_drop=0.5)
    mc._call = 100
    with torch.no_grad():
        greedy_shared, _ = mc.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    w = min(greedy_shared.shape[1], ng)
    assert not torch.equal(greedy_shared[:, :w], greedy_a[:, :w])


def test_single_step_backward_vs_oracle_autograd():
    """xg_step_bwd (SURVEY.md 8b export list): gradients of one LSTMCore_two_layer_gate step (sub_modules.py:671-687) wrt
    the old state, V, v2a(V), pos and every lstmcore / embed parameter == autograd over the oracle's core_step, with a held
    row (xt_mask = 0) in the batch."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _grads_struct, _stream, _ws_ptr
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d)
    B, K, R, E, A = d.B, d.K, d.R, d.E, d.A
    Vn = pg.uniform("sb.V", (B, K, R), 7, 0.0, 1.0)
    posn = pg.uniform("sb.pos", (B, R), 7, -1.0, 1.0)
    stn = pg.uniform("sb.st", (4, B, R), 7, -0.5, 0.5)
    wn = pg.uniform("sb.w", (4, B, R), 7, -1.0, 1.0)                  # d(loss)/d(new state)
    tok = pg.randint("sb.tok", (B,), 7, 2, d.V)
    mk = np.ones((B,), np.float32); mk[2] = 0.0; mk[7] = 0.0
    # ---- oracle
    P = xo.to_torch_params(Pn, requires_grad=True)
    Vt = torch.from_numpy(Vn).requires_grad_(True)
    vp = (Vt.detach() @ P["lstmcore.v2a.weight"].detach().t() + P["lstmcore.v2a.bias"].detach()).requires_grad_(True)
    post = torch.from_numpy(posn).requires_grad_(True)
    st = [torch.from_numpy(stn[i].copy()).requires_grad_(True) for i in range(4)]
    xt = P["embed.weight"][torch.from_numpy(tok)]
    out, ns, alpha_o = xo.core_step(P, xt, torch.from_numpy(mk).unsqueeze(1), Vt, post, [(st[0], st[1]), (st[2], st[3])], vproj=vp)
    wt = torch.from_numpy(wn)
    loss = (ns[0][0] * wt[0]).sum() + (ns[0][1] * wt[1]).sum() + (ns[1][0] * wt[2]).sum() + (ns[1][1] * wt[3]).sum()
    loss.backward()
    # ---- HIP
    model = make_model(d, P=Pn, train=True)
    model.flat_grads().zero_()
    dd = model._dims(B, K, 1)
    ps = model._params_struct()
    run = model._run(True)
    g, gs = _grads_struct(model, "cuda")
    assert g is None                                                    # grads accumulate into the bound flat buffer
    L = nv.lib()
    Vd, posd = torch.from_numpy(Vn).cuda(), torch.from_numpy(posn).cuda()
    vpd = vp.detach().cuda().contiguous()
    tokd, mkd = torch.from_numpy(tok).cuda(), torch.from_numpy(mk).cuda()
    state = torch.from_numpy(stn).cuda().contiguous()
    ws = model._pool.shared(dd, Vd.device)
    wp, wnb = _ws_ptr(ws)
    alpha = torch.zeros(B, K, device="cuda")
    nv.check(L.xg_step_fwd(_stream(), C.byref(dd), C.byref(ps), nv.ptr(tokd), nv.ptr(mkd), nv.ptr(Vd), nv.ptr(vpd), nv.ptr(posd),
                           C.byref(run), 3, wp, wnb, nv.ptr(state), None, nv.ptr(alpha)), "xg_step_fwd")
    np.testing.assert_allclose(state[2].cpu().numpy(), out.detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(alpha.cpu().numpy(), alpha_o.detach().numpy(), atol=2e-6)
    dst_new = torch.from_numpy(wn).cuda().contiguous()
    dst = torch.full((4, B, R), 7.0, device="cuda")                     # overwritten
    dV = torch.zeros(B, K, R, device="cuda"); dvp = torch.zeros(B, K, A, device="cuda"); dpos = torch.zeros(B, R, device="cuda")
    nv.check(L.xg_step_bwd(_stream(), C.byref(dd), C.byref(ps), C.byref(gs), nv.ptr(tokd), nv.ptr(mkd), nv.ptr(Vd), nv.ptr(vpd),
                           nv.ptr(posd), C.byref(run), 3, wp, wnb, nv.ptr(state), nv.ptr(dst_new), nv.ptr(dst), nv.ptr(dV),
                           nv.ptr(dvp), nv.ptr(dpos)), "xg_step_bwd")
    torch.cuda.synchronize()

    def close(got, want, name):
        want = want.numpy()
        err = np.abs(got.cpu().numpy() - want).max()
        assert err <= 2e-6 + 2e-3 * np.abs(want).max(), (name, float(err), float(np.abs(want).max()))
    for i in range(4):
        close(dst[i], st[i].grad, "dstate[%d]" % i)
    close(dV, Vt.grad, "dV"); close(dvp, vp.grad, "dvproj"); close(dpos, post.grad, "dpos")
    for name, prm in model.named_parameters():
        if not (name.startswith("lstmcore.") or name == "embed.weight") or name in ("lstmcore.a2w.bias", "lstmcore.v2a.weight", "lstmcore.v2a.bias"):
            continue
        want = P[name].grad if P[name].grad is not None else torch.zeros_like(P[name])
        close(prm.grad, want, name)


# ---------------------------------------------------------------- split-bf16 arithmetic of the per-step products (gemm_mode 3)
@pytest.mark.parametrize("tag,ragged", [("tiny", True), ("mid", True), ("c1", False), ("c1", True)])
def test_split_bf16_step_products_xe_vs_oracle(tag, ragged):
    """precision='bf16x3' (XgRun.gemm_mode 3): the large products AND the per-step products (xg_step.hip, PREC 2: three bf16
    planes of the packed fp32 weights and of the staged activations, six plane products per 16-deep block) are fp32-class:
    the same tolerances as the exact-fp32 path -- loss within 1e-4 (north_star), log-probs, every gradient."""
    d = pg.make_dims(**CFG[tag])
    P, lo, co, lxe_o, lcls_o, running = run_oracle_xe(d, ragged)
    model, lh, ch, lxe_h, lcls_h = run_hip_xe(d, ragged, precision="bf16x3")
    assert abs(lxe_h - lxe_o) < 1e-4, (lxe_h, lxe_o)
    assert abs(lcls_h - lcls_o) < 1e-4
    np.testing.assert_allclose(lh, lo, atol=3e-4, rtol=0)
    np.testing.assert_allclose(ch, co, atol=1e-4, rtol=0)
    assert_grads_close(model, oracle_grads(P))


@pytest.mark.parametrize("name,tag,ragged", [("greedy_tiny.npz", "tiny", False), ("greedy_c1.npz", "c1", False),
                                              ("greedy_c1_ragged.npz", "c1", True), ("greedy_c1_eos.npz", "c1", False),
                                              ("beam_c1.npz", "c1", False)])
def test_split_bf16_greedy_token_for_token_vs_reference(name, tag, ragged):
    """Every greedy golden of the reference (and the beam-size-1 decode of the beam golden's inputs against the exact-fp32 HIP
    path), decoded with the split-bf16 step products: the same tokens."""
    from tests.util import EOS_CASE, eos_params
    d = pg.make_dims(**CFG[tag])
    eos = name == "greedy_c1_eos.npz"
    Pn = eos_params(d) if eos else None
    if name.startswith("greedy") and not eos:
        Pn = pg.make_params(d, logit_gain=float(load_golden(name)["logit_gain"]))
    x = to_dev(pg.make_inputs(d, seed=EOS_CASE["input_seed"] if eos else 0, ragged=ragged))
    model = make_model(d, P=Pn, train=False, precision="bf16x3")
    with torch.no_grad():
        seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
    if name.startswith("beam"):
        ref_model = make_model(d, P=Pn, train=False)
        with torch.no_grad():
            rs, rl = ref_model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
        want_seq, want_lp = rs.cpu().numpy(), rl.cpu().numpy()
    else:
        g = load_golden(name)
        want_seq, want_lp = g["seq"], g["seqLogprobs"]
    seq, slp = seq.cpu().numpy(), slp.cpu().numpy()
    assert seq.shape == want_seq.shape
    assert np.array_equal(seq, want_seq), np.argwhere(seq != want_seq)
    np.testing.assert_allclose(slp, want_lp, atol=3e-4)


def test_split_bf16_presplit_weight_planes_equal_the_in_register_split():
    """Round 5: the packed recurrent weights of the split-bf16 mode are three bf16 planes split ONCE per update (xg_pack_weights
    dtype 2) instead of fp32 tiles split in registers by every launch.  Same split, same MFMA order: the teacher-forced forward
    (log-probabilities, category log-probabilities) and a greedy rollout must be bit-identical between the two tile formats."""
    d = pg.make_dims(**CFG["mid"])
    x = to_dev(pg.make_inputs(d, seed=3, ragged=True))
    args = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], x["seq"], x["seq_mask"])
    outs = []
    for over in (None, 0):
        model = make_model(d, precision="bf16x3", train=False)
        model._packed_dtype_override = over
        with torch.no_grad():
            logp, cat = model(*args)
            seq, slp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
        torch.cuda.synchronize()
        assert model._packed_dtype() == (2 if over is None else 0)
        outs.append((logp.clone(), cat.clone(), seq.clone(), slp.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_split_bf16_raw_step_equals_exact_fp32_step():
    """xg_step_fwd at 128 rows (the benchmarked launch group) in gemm_mode 3 against gemm_mode 0: new state within 2e-6."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _stream, _ws_ptr
    import ctypes as C
    d = pg.make_dims(**dict(CFG["c1"], B=128))
    Pn = pg.make_params(d)
    x = to_dev(pg.make_inputs(d, seed=0))
    outs = []
    for precision in ("fp32", "bf16x3"):
        model = make_model(d, P=Pn, train=False, precision=precision)
        with torch.no_grad():
            V = model.encode(x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
            st = model.init_hidden(V, x["feat_mask"])
            state = torch.cat([st[0][0], st[0][1], st[1][0], st[1][1]], 0).contiguous()
            dd = model._dims(d.B, d.K, 1)
            ps, run = model._params_struct(), model._run(False)
            vproj = torch.empty(d.B, d.K, model.att_size, device="cuda")
            nv.check(nv.lib().xg_vproj(_stream(), C.byref(dd), C.byref(ps), nv.ptr(V), nv.ptr(vproj), C.byref(run)), "xg_vproj")
            ws = model._pool.shared(dd, V.device)
            wp, wn = _ws_ptr(ws)
            tok = x["seq"][:, 1].contiguous()
            for _ in range(3):
                nv.check(nv.lib().xg_step_fwd(_stream(), C.byref(dd), C.byref(ps), nv.ptr(tok), None, nv.ptr(V), nv.ptr(vproj),
                                              nv.ptr(x["pos_feats"]), C.byref(run), 0, wp, wn, nv.ptr(state), None, None), "xg_step_fwd")
            torch.cuda.synchronize()
        outs.append(state.cpu().numpy())
    np.testing.assert_allclose(outs[1], outs[0], atol=5e-6, rtol=0)


def test_paired_rollout_over_videos_equals_the_repeated_batch_entry_point():
    """xg_rollout_pair_videos (the m videos handed over once, encoder run once, BatchNorm updated twice in the library) against
    xg_rollout_pair on the caller-repeated 2m-row batch: same tokens, same log-probs, same early-exit widths."""
    import ctypes as C
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _stream, _ws_ptr
    d = pg.make_dims(**CFG["mid"])
    Pn = pg.make_params(d, logit_gain=1.0)
    x = to_dev(pg.make_inputs(d, seed=0, ragged=True))
    u = torch.from_numpy(pg.uniform("uni2", (d.L + 1, d.B), 78)).cuda()
    model = make_model(d, P=Pn, train=True)
    with torch.no_grad():
        gen, slp, greedy, n = model.sample_pair(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"uniforms": u})
    torch.cuda.synchronize()
    ref = make_model(d, P=Pn, train=True)
    B, T = d.B, d.L + 1
    d2 = ref._dims(2 * B, d.K, T)
    ws2 = ref._pool.shared(d2, x["feats_rgb"].device)
    wp2, wn2 = _ws_ptr(ws2)
    b2, keep = ref._batch(torch.cat([x["feats_rgb"]] * 2), torch.cat([x["feats_opfl"]] * 2), torch.cat([x["feat_mask"]] * 2),
                          torch.cat([x["pos_feats"]] * 2))
    seq = torch.zeros(2 * B, T - 1, dtype=torch.int64, device="cuda")
    lp = torch.zeros(2 * B, T - 1, dtype=torch.float32, device="cuda")
    nn_ = torch.zeros(2, dtype=torch.int32, device="cuda")
    ps, run = ref._params_struct(), ref._run(False)
    nv.check(nv.lib().xg_rollout_pair(_stream(), C.byref(d2), C.byref(ps), C.byref(nv.XgBnState()), C.byref(b2), C.byref(run), B,
                                      nv.ptr(u), 1.0, wp2, wn2, nv.ptr(seq), nv.ptr(lp), nv.ptr(nn_)), "xg_rollout_pair")
    torch.cuda.synchronize()
    assert torch.equal(n.cpu(), nn_.cpu())
    w = int(n[0]), int(n[1])
    assert torch.equal(seq[:B, :w[0]].cpu(), gen[:, :w[0]].cpu()) and torch.equal(seq[B:, :w[1]].cpu(), greedy[:, :w[1]].cpu())
    np.testing.assert_allclose(lp[:B, :w[0]].cpu().numpy(), slp[:, :w[0]].cpu().numpy(), atol=2e-6)


@pytest.mark.parametrize("precision,cfg,rows", [("fp32", "c1", 128), ("bf16x3", "c1", 128), ("bf16", "c1", 128), ("fp32", "c1", 64),
                                                ("bf16x3", "c1", 64), ("fp32", "c1", 40), ("bf16", "c5", 128), ("bf16x3", "c5", 128),
                                                ("fp32", "c5", 64)])
def test_in_place_steps_are_bitwise_reproducible(precision, cfg, rows):
    """Three consecutive xg_step_fwd calls on an in-place state, twelve times over: every repetition must give the same bits.
    Round 4 found single elements of the attention context differing from run to run in the split-bf16 mode (a compiler-formed
    v_pk_fma_f32 with operand-select modifiers, see __graft_entry__.FLAGS); the accumulation order of the step is fixed, so
    anything but identical bits is a bug.  Shapes: 128 rows (the 8-wave launches that carry the fused attention beside cell
    tiles), 64 and 40 rows (two row tiles, one of them ragged), hidden 1024 / 40 frames (4-wave workgroups), all three
    arithmetic modes."""
    import ctypes as C
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd.model import _stream, _ws_ptr
    d = pg.make_dims(**dict(CFG[cfg], B=rows))
    x = to_dev(pg.make_inputs(d, seed=0))
    model = make_model(d, train=False, precision=precision)
    with torch.no_grad():
        V = model.encode(x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
        st = model.init_hidden(V, x["feat_mask"])
        state0 = torch.cat([st[0][0], st[0][1], st[1][0], st[1][1]], 0).contiguous()
        dd = model._dims(d.B, d.K, 1)
        ps, run = model._params_struct(), model._run(False)
        vproj = torch.empty(d.B, d.K, model.att_size, device="cuda")
        nv.check(nv.lib().xg_vproj(_stream(), C.byref(dd), C.byref(ps), nv.ptr(V), nv.ptr(vproj), C.byref(run)), "xg_vproj")
        ws = model._pool.shared(dd, V.device)
        wp, wn = _ws_ptr(ws)
        tok = x["seq"][:, 1].contiguous()
        first = None
        for rep in range(12):
            s = state0.clone()
            for _ in range(3):
                nv.check(nv.lib().xg_step_fwd(_stream(), C.byref(dd), C.byref(ps), nv.ptr(tok), None, nv.ptr(V), nv.ptr(vproj),
                                              nv.ptr(x["pos_feats"]), C.byref(run), 0, wp, wn, nv.ptr(s), None, None), "xg_step_fwd")
            torch.cuda.synchronize()
            if first is None:
                first = s.clone()
            else:
                assert torch.equal(s, first), (precision, cfg, rows, rep, float((s - first).abs().max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_greedy_rollout_is_reproducible(precision):
    """A whole greedy rollout (encoder, 20 core steps with the vocabulary product and the token choice per step) three times on
    the same inputs.  fp32 arithmetic: identical tokens and identical log-probabilities, bit for bit.  Split-bf16: the tiled
    products of that path split deep reductions across workgroups and add the partial tiles with fp32 atomics in arrival order
    (xg_gemm_bf16.hip: splitk), so the encoder's output moves in its last bit from run to run (1.5e-7 measured): identical
    tokens, log-probabilities within 2e-5.  (Plain bf16 rounds those differences up to 1e-4 and a near-tie may flip a token:
    not asserted)"""
    d = pg.make_dims(**dict(CFG["c1"], B=64))
    x = to_dev(pg.make_inputs(d, seed=0))
    model = make_model(d, train=False, precision=precision)
    first = None
    for rep in range(3):
        with torch.no_grad():
            seq, lp = model.sample(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], x["pos_feats"], {"sample_max": 1})
        torch.cuda.synchronize()
        if first is None:
            first = (seq.clone(), lp.clone())
        elif precision == "fp32":
            assert torch.equal(seq, first[0]) and torch.equal(lp, first[1]), (precision, rep)
        else:
            assert torch.equal(seq, first[0]), (precision, rep)
            np.testing.assert_allclose(lp.cpu().numpy(), first[1].cpu().numpy(), atol=2e-5, rtol=0)


# ---------------------------------------------------------------- the eval-mode goldens with a model built with drop_prob_lm = 0.5
# The reference evaluates a model built from the saved options (drop_prob_lm = 0.5) and switched to eval() (eval.py:57-73):
# XgRun then carries train = 0, drop_p = 0.5, and no dropout site may act.  The same assertions as the p = 0 tests above.
@pytest.mark.parametrize("name,tag,ragged", [("greedy_tiny.npz", "tiny", False), ("greedy_c1.npz", "c1", False),
                                              ("greedy_c1_ragged.npz", "c1", True)])
def test_eval_dropout_half_greedy_token_for_token_vs_reference(name, tag, ragged):
    test_greedy_token_for_token_vs_reference(name, tag, ragged, p_drop=0.5)


def test_eval_dropout_half_greedy_with_natural_eos_vs_reference():
    test_greedy_with_natural_eos_token_for_token_vs_reference(p_drop=0.5)


def test_eval_dropout_half_batchnorm_vs_golden():
    test_eval_mode_batchnorm_vs_golden(p_drop=0.5)


@pytest.mark.parametrize("tag", ["tiny", "c1"])
def test_eval_dropout_half_beam_search_vs_reference_golden(tag):
    test_beam_search_vs_reference_golden(tag, p_drop=0.5)


@pytest.mark.parametrize("beam", [1, 3])
def test_eval_dropout_half_eval_split_vs_oracle_and_beam_golden(beam):
    test_eval_split_vs_oracle_and_beam_golden(beam, p_drop=0.5)
