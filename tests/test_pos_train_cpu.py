"""CPU checks of POS generator training: the train-mode oracle (tests/pos_train_oracle.py) against the reference's own train-mode
outputs (tests/golden/pos_train_*.npz), the C ABI of include/xgate_pos_train.h (exports, struct sizes, error codes without a GPU)
and the learning-rate schedule of pos_train.PosTrainer.  No compute on a GPU."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.util import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


def load_case(name):
    cfg, kw, p, seed = pto.TRAIN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    return d, po.make_params(d), po.make_running(d), po.make_inputs(d, **kw), p, seed, dict(np.load(os.path.join(GOLD, "pos_train_%s.npz" % name)))


@pytest.mark.parametrize("name", list(pto.TRAIN_CASES))
def test_train_oracle_matches_reference_goldens(name):
    d, P, run, x, p, seed, g = load_case(name)
    loss, grads, stats, run_new, out = pto.loss_and_grads(d, P, run, x, p, seed)
    assert out.shape[1] == int(g["tf_T"])
    assert abs(loss - float(g["loss"])) < 1e-5 * max(1.0, abs(float(g["loss"])))
    assert not pto.golden_grad_misses(grads, g)
    for m in ("rgb", "opfl"):
        np.testing.assert_allclose(stats[m + "_mean"], g["bn_mean/" + m], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(stats[m + "_var"], g["bn_var/" + m], rtol=1e-5, atol=1e-6)
        for b in ("running_mean", "running_var"):
            np.testing.assert_allclose(run_new["two_fc_encoder.visual_emb_%s.1.%s" % (m, b)], g["run/%s/%s" % (m, b)], rtol=1e-5,
                                       atol=1e-6)


def test_dropout_case_differs_from_p0():
    """The p = 0.5 fixture really drops: its loss is not the same inputs' p = 0 loss."""
    d, P, run, x, p, seed, g = load_case("drop")
    assert p > 0
    loss0 = pto.loss_and_grads(d, P, run, x, 0.0, seed)[0]
    assert abs(loss0 - float(g["loss"])) > 1e-3


def test_train_oracle_trajectory_matches_reference_adam():
    cfg, kw = pto.TRAJ_CASE
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d), po.make_running(d), po.make_inputs(d, **kw)
    g = dict(np.load(os.path.join(GOLD, "pos_train_traj.npz")))
    state, P0 = {}, dict(P)
    for it in range(pto.TRAJ_STEPS):
        loss, grads, _, run, _ = pto.loss_and_grads(d, P, run, x)
        assert abs(loss - g["losses"][it]) < 1e-5
        P = pto.clip_adam(P, grads, state, it + 1)
        assert not pto.traj_misses(P, P0, g, it)


def _train_header():
    with open(os.path.join(ROOT, "include", "xgate_pos_train.h")) as f:
        return f.read()


def test_library_exports_every_xgpt_function(built):
    syms = sorted(set(re.findall(r"\b(xgpt_[a-z_0-9]+)\s*\(", _train_header())))
    assert syms == ["xgpt_backward", "xgpt_forward_train", "xgpt_version", "xgpt_workspace_bytes"]
    lib = ctypes.CDLL(built)
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s


def test_train_struct_sizes_and_version(built, tmp_path):
    from controllable_xgating_amd import _native_pos_train as npt
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xgate_pos_train.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d\\n", sizeof(XgptRun), offsetof(XgptRun, drop_p), offsetof(XgptRun, seed), '
                   'offsetof(XgptRun, bn_momentum), XGPT_VERSION, XGP_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sz, o1, o2, o3, ver, pver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert sz == ctypes.sizeof(npt.XgptRun)
    assert (o1, o2, o3) == (npt.XgptRun.drop_p.offset, npt.XgptRun.seed.offset, npt.XgptRun.bn_momentum.offset)
    L = npt.lib()
    assert ver == npt.XGPT_VERSION == L.xgpt_version()
    assert pver == 1


def test_train_bad_arguments_return_error_codes_without_a_gpu(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_train as npt
    L = npt.lib()
    d = po.make_dims(**po.POS_CFG["tiny"])
    dims = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, d.L + 1)
    no_t = npos.XgpDims(d.B, d.K, d.R, d.A, d.E, d.C, d.F1, d.F2, 0)
    assert L.xgpt_workspace_bytes(ctypes.byref(dims)) > 0
    assert L.xgpt_workspace_bytes(ctypes.byref(no_t)) == 0
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    G = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    run = npt.XgptRun(1, 0.5, 7, 0.1)
    B = ctypes.byref
    # a too-small workspace -> XG_EWORKSPACE; missing pointers / bad run / bad T' -> XG_EINVAL; nothing is dereferenced
    assert L.xgpt_forward_train(None, B(dims), B(P), B(bn), B(run), fake, fake, fake, fake, fake, fake, fake, fake, 8) == -4
    assert L.xgpt_forward_train(None, B(dims), B(P), B(bn), None, fake, fake, fake, fake, fake, fake, fake, fake, 1 << 40) == -1
    assert L.xgpt_forward_train(None, B(dims), B(P), B(bn), B(run), fake, fake, fake, None, fake, fake, fake, fake, 1 << 40) == -1
    bad_run = npt.XgptRun(1, 1.0, 7, 0.1)
    assert L.xgpt_forward_train(None, B(dims), B(P), B(bn), B(bad_run), fake, fake, fake, fake, fake, fake, fake, fake, 1 << 40) == -1
    assert L.xgpt_backward(None, B(dims), B(P), B(G), B(run), fake, fake, fake, 3, fake, fake, 8) == -4
    assert L.xgpt_backward(None, B(dims), B(P), B(G), B(run), fake, fake, fake, 0, fake, fake, 1 << 40) == -1
    assert L.xgpt_backward(None, B(dims), B(P), B(G), B(run), fake, fake, fake, d.L + 2, fake, fake, 1 << 40) == -1
    G0 = npos.XgpParams(*([fake] * (len(npos.PARAM_NAMES) - 1) + [None]))
    assert L.xgpt_backward(None, B(dims), B(P), B(G0), B(run), fake, fake, fake, 3, fake, fake, 1 << 40) == -1


def test_train_refuses_shapes_beyond_the_attention_backward(built):
    """T K * 4 > XGPT_MAX_TK_BYTES (60000): the attention backward after the step loop cannot run it, so the workspace query
    returns 0 and both entry points return XG_EINVAL before anything is enqueued (before, the backward failed half-way, after
    adding most gradients, and the forward had already moved the running statistics)."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_pos as npos
    from controllable_xgating_amd import _native_pos_train as npt
    assert re.search(r"#define XGPT_MAX_TK_BYTES 60000\b", _train_header())
    L = npt.lib()
    B = ctypes.byref
    T = 29                                               # seq_length 28
    assert L.xgpt_workspace_bytes(B(npos.XgpDims(1, 517, 8, 8, 4, 3, 4, 4, T))) > 0       # 29 * 517 * 4 = 59972
    dims = npos.XgpDims(1, 600, 8, 8, 4, 3, 4, 4, T)                                       # 29 * 600 * 4 = 69600
    # first: a library without the check stops the test here, before any call below could enqueue work on fake pointers
    assert L.xgpt_workspace_bytes(B(dims)) == 0
    fake = 16
    P = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    G = npos.XgpParams(*([fake] * len(npos.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    run = npt.XgptRun(1, 0.0, 7, 0.1)
    assert L.xgpt_forward_train(None, B(dims), B(P), B(bn), B(run), fake, fake, fake, fake, fake, fake, fake, fake, 1 << 40) == -1
    assert L.xgpt_backward(None, B(dims), B(P), B(G), B(run), fake, fake, fake, T, fake, fake, 1 << 40) == -1


def _reference_lr(opt, epoch):
    """starttrain_trainpos.py:98-105, restated."""
    if epoch > opt.learning_rate_decay_start and opt.learning_rate_decay_start >= 0:
        frac = int((epoch - opt.learning_rate_decay_start) / opt.learning_rate_decay_every)
        return opt.learning_rate * opt.learning_rate_decay_rate ** frac
    return opt.learning_rate


@pytest.mark.parametrize("start,every,rate", [(0, 3, 0.8), (-1, 3, 0.8), (5, 2, 0.5)])
def test_pos_trainer_lr_schedule_matches_reference(start, every, rate):
    from controllable_xgating_amd.pos_train import PosTrainer

    class _Opt:
        lr = None

        def set_lr(self, lr):
            self.lr = lr

    opt = argparse.Namespace(learning_rate=4e-4, learning_rate_decay_start=start, learning_rate_decay_every=every,
                             learning_rate_decay_rate=rate, grad_clip=0.1)
    tr = PosTrainer.__new__(PosTrainer)
    tr.opt, tr.optimizer, tr.model = opt, _Opt(), argparse.Namespace(ss_prob=0.0)
    for epoch in range(12):
        tr.start_epoch(epoch)
        assert tr.optimizer.lr == pytest.approx(_reference_lr(opt, epoch), rel=1e-12)
        assert opt.current_lr == tr.optimizer.lr


def test_train_mode_on_cpu_raises_not_implemented():
    from controllable_xgating_amd.pos import PosModel
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1,
                                    drop_prob_lm=0.5, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2))
    x = {k: torch.from_numpy(v) for k, v in po.make_inputs(d).items()}
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    m.train()
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m(x["feats_rgb"], x["feats_opfl"], x["feat_mask"], None, None, cap_r, new_mask)


def test_pos_trainer_update_best_saves_and_counts_patience(tmp_path):
    from controllable_xgating_amd.pos import PosModel
    from controllable_xgating_amd.pos_train import PosTrainer
    d = po.make_dims(**po.POS_CFG["tiny"])
    m = PosModel(argparse.Namespace(category_size=d.C, input_encoding_size=d.E, rnn_size=d.R, att_size=d.A, num_layers=1,
                                    drop_prob_lm=0.5, seq_length=d.L, feat_size=d.F1, feat_size2=d.F2))
    opt = argparse.Namespace(learning_rate=4e-4, patience=2)
    tr = PosTrainer.__new__(PosTrainer)                  # (no optimizer: ClipAdam needs the GPU)
    tr.model, tr.opt, tr.iteration, tr.epoch, tr.best_val_score, tr.patience = m, opt, 5, 1, None, 0
    path = str(tmp_path / "ckpt")
    assert tr.update_best(path, 2.0) is False            # first score: best, saved
    assert tr.best_val_score == -2.0 and tr.patience == 0
    sd = torch.load(os.path.join(path, "model-best.pth"))
    assert list(sd) == po.state_dict_keys(d)
    assert torch.load(os.path.join(path, "infos-best.pkl"), weights_only=False)["val_score"] == -2.0
    with torch.no_grad():
        m.logit.bias.fill_(3.0)
    assert tr.update_best(path, 2.5) is False            # worse: patience 1, the best checkpoint is kept
    assert tr.patience == 1 and tr.best_val_score == -2.0
    assert float(torch.load(os.path.join(path, "model-best.pth"))["logit.bias"].abs().max()) == 0.0
    assert tr.update_best(path, 1.5) is False            # better: saved again, patience reset
    assert tr.patience == 0 and tr.best_val_score == -1.5
    assert float(torch.load(os.path.join(path, "model-best.pth"))["logit.bias"][0]) == 3.0
    assert tr.update_best(path, 1.6) is False
    assert tr.update_best(path, 1.7) is True             # patience 2 reached: stop


def test_prepare_pos_targets_unchecked_matches_checked():
    from controllable_xgating_amd.pos import prepare_pos_targets
    d = po.make_dims(**po.POS_CFG["mid"])
    x = po.make_inputs(d, seed=2, ragged=True)
    cap, cm = torch.from_numpy(x["cap_classes"]), torch.from_numpy(x["class_mask"])
    a = prepare_pos_targets(cap, cm)
    b = prepare_pos_targets(cap, cm, check=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    bad = cm.clone()
    bad[1] = 0
    with pytest.raises(ValueError):
        prepare_pos_targets(cap, bad)
    assert bool((prepare_pos_targets(cap, bad, check=False)[1][1] == 1).all())
