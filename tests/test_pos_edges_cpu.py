"""CPU checks behind tests/test_gpu_pos_edges.py: the named edge cases reach every kernel branch of the POS entry points (as
tests/pos_edge_cases.branches restates the launchers' selection), and the float64 oracle the GPU module compares with reproduces
the reference's fixtures.  No compute on a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import pos_edge_cases as pe
from tests import pos_oracle as po
from tests.util import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("mode,rows", [("eval", pe.EVAL_ROWS), ("train", pe.TRAIN_ROWS)])
def test_named_cases_reach_every_branch(mode, rows):
    reached = {}
    for name in pe.EDGE_CASES:
        for r in pe.branches(pe.case_dims(name), mode):
            reached.setdefault(r, []).append(name)
    assert set(reached) == rows, (mode, sorted(rows - set(reached)), sorted(set(reached) - rows))


def test_fixture_shapes_reach_none_of_the_branches():
    """The five POS_CFG shapes (what the suite ran before the edge cases) take none of these branches; the named cases are the
    only tests that do.  (If a fixture shape starts reaching one, this list of rows is out of date.)"""
    for cfg in po.POS_CFG.values():
        assert not pe.branches(cfg, "eval") and not pe.branches(cfg, "train"), cfg


def test_branch_conditions_at_their_boundaries():
    base = pe.case_dims("c64")
    assert "4" not in pe.branches(base, "eval") and "4" in pe.branches(dict(base, C=65), "eval")
    assert "5" not in pe.branches(base, "train") and "5b" not in pe.branches(dict(base, C=128), "train")
    assert "5b" in pe.branches(dict(base, C=129), "train")
    assert "3" not in pe.branches(dict(base, R=1024), "eval") and "3" in pe.branches(dict(base, R=1028), "eval")
    assert "6" not in pe.branches(dict(base, B=256), "eval") and "6" in pe.branches(dict(base, B=257), "train")
    assert "10" not in pe.branches(dict(base, L=31), "train") and "10" in pe.branches(dict(base, L=32), "train")
    k = dict(base, R=512, A=1536)
    assert "2" not in pe.branches(dict(k, K=32), "eval") and "2" in pe.branches(dict(k, K=33), "eval")
    assert "9b" not in pe.branches(dict(k, K=32), "train") and "9b" in pe.branches(dict(k, K=48), "train")
    assert "9c" in pe.branches(dict(k, K=49), "train")
    bn = dict(base, R=16, B=128, K=32)
    assert not {"8a", "8b"} & pe.branches(bn, "train")
    assert "8a" in pe.branches(dict(bn, B=160), "train") and "8b" in pe.branches(dict(bn, B=161), "train")


def test_every_fuzz_case_within_the_train_limit_and_every_variant_drawn():
    ds = [pe.fuzz_dims(i) for i in range(12)]
    assert all((d["L"] + 1) * d["K"] * 4 <= 60000 for d in ds)
    v = [pe.fuzz_variant(i, d) for i, d in enumerate(ds)]
    assert any(r for r, _, _ in v) and any(p > 0 for _, p, _ in v) and sum(e for _, _, e in v) == 3
    for name, d in pe.EDGE_CASES.items():
        assert (d["L"] + 1) * d["K"] * 4 <= 60000, name


@pytest.mark.parametrize("name", ["tiny", "eos"])
def test_float64_oracle_reproduces_the_goldens(name):
    cfg, kw, eos = po.GOLDEN_CASES[name]
    d = po.make_dims(**po.POS_CFG[cfg])
    P, run, x = po.make_params(d, eos=eos), po.make_running(d), po.make_inputs(d, **kw)
    g = dict(np.load(os.path.join(GOLD, "pos_%s.npz" % name)))
    f64 = torch.float64
    Pt, rt = po.to_torch(P, f64), po.to_torch(run, f64)
    assert all(v.dtype == f64 for v in Pt.values())
    fr, fo, fm = (torch.from_numpy(x[k]).to(f64) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    out = po.forward_tf(Pt, rt, fr, fo, fm, cap_r, new_mask.to(f64))
    assert out.dtype == f64 and out.shape[1] == int(g["tf_T"])
    np.testing.assert_allclose(out.numpy(), g["tf_logp"], atol=2e-5)
    seq, slp, states, masks, _ = po.sample_greedy(Pt, rt, fr, fo, fm, d.L)
    assert states.dtype == f64 and masks.dtype == f64
    assert np.array_equal(seq.numpy(), g["seq"])
    np.testing.assert_allclose(slp.numpy(), g["seqLogprobs"], atol=2e-5)
    np.testing.assert_allclose(states.numpy()[:, :, :g["states"].shape[2]], g["states"], atol=2e-5)
