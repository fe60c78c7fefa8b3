"""The POS generator's kernel branches that the fixture shapes never reach, against the float64 oracle (tests/pos_oracle.py,
tests/pos_train_oracle.py in eager torch on the same GPU), in eval mode (teacher-forced logp and loss, the greedy rollout) and in
train mode (loss, logp, every gradient, the running statistics).  tests/pos_edge_cases.py names the branches and the cases; its
`branches()` restates each launcher's selection and tests/test_pos_edges_cpu.py checks that the named cases reach all of them:

   1  pos_attn_kernel<false> (A % 4 != 0)                  6  pos_first_zero_col_kernel's strided row loop (B > 256)
   2  pos_attn_kernel without the V prefetch               7  step products on the skinny launcher's LDS-staged kernel (R % 4)
   3  R > 1024: second pass of the cell kernels' j-loops   8  bn_train_fwd_kernel<20>; xgk_bn_stats + xgk_bn_apply at R % 16 == 0
   4  the eval cell's serial head (C > 64)                 9  xgk_attn_fwd generic; xgk_attn_bwd <48> and generic forms
   5  the train cell's 64-wide chunk loops (C > 64, 128)  10  xgk_attn_post_dV's two-pass path (Tp > 32)

Plus the targeted checks: T' with B > 256, greedy ties in both head forms, T' = 1 / 2, and train shapes whose attention backward
the library cannot run (refused before anything moves)."""
import numpy as np
import pytest
import torch

from tests import pos_edge_cases as pe
from tests import pos_oracle as po
from tests import pos_train_oracle as pto
from tests.test_gpu_pos import check_against, run_model
from tests.test_gpu_pos import pos_model as eval_model
from tests.test_gpu_pos_train import grads_of, pos_model as train_model, running_of, train_step
from tests.util import grad_misses

pytestmark = pytest.mark.gpu
F64 = torch.float64


def oracle_eval(d, P, run, x, device="cuda"):
    """The eval-mode oracle in float64 (on the GPU: eager torch): check_against's reference dict and the (n, B) top-1 / top-2
    margins."""
    Pt, rt = po.to_torch(P, F64, device), po.to_torch(run, F64, device)
    fr, fo, fm = (torch.from_numpy(x[k]).to(device, F64) for k in ("feats_rgb", "feats_opfl", "feat_mask"))
    cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
    cap_r, new_mask = cap_r.to(device), new_mask.to(device, F64)
    out = po.forward_tf(Pt, rt, fr, fo, fm, cap_r, new_mask)
    loss = po.criterion(out, cap_r, new_mask, torch.from_numpy(x["class_mask"]).to(device, F64))
    try:
        seq, slp, states, masks, lps = po.sample_greedy(Pt, rt, fr, fo, fm, d.L)
    except RuntimeError as e:       # (torch.stack of no steps: every row chose EOS first, which the reference cannot run either)
        raise AssertionError("every row picks EOS at the first choice: this case needs another input seed") from e
    assert seq.shape[1] >= 1
    top2 = torch.topk(lps, 2, dim=2).values
    o = dict(tf_logp=out.cpu().numpy(), loss=float(loss), seq=seq.cpu().numpy(), seqLogprobs=slp.cpu().numpy(),
             states=states.cpu().numpy(), masks=masks.cpu().numpy())
    return o, (top2[:, :, 0] - top2[:, :, 1]).cpu().numpy()


def check_eval(d, P, run, x):
    h = run_model(eval_model(d, P, run), x)
    o, margin = oracle_eval(d, P, run, x)
    assert h["tf_logp"].shape == o["tf_logp"].shape
    check_against(h, o, margin)
    if (margin >= 1e-3).all():      # no near-tie anywhere: the rollouts have the same length n
        assert h["seq"].shape == o["seq"].shape and np.array_equal(h["seq"], o["seq"])
    return h, o


def check_train(d, P, run, x, p, seed):
    m = train_model(d, P, run, p, seed)
    loss, out = train_step(m, x)
    lo, go, _, ro, out_o = pto.loss_and_grads(d, P, run, x, p, seed, dtype=F64, device="cuda")
    assert out.shape == out_o.shape
    assert abs(loss - lo) < 1e-4, (loss, lo)
    np.testing.assert_allclose(out.cpu().numpy(), out_o, atol=3e-4)
    gh = grads_of(m)
    miss = grad_misses(gh, go, skip=pto.ZERO_GRAD)
    assert not miss, miss
    for n in pto.ZERO_GRAD:
        assert np.abs(gh[n]).max() < 1e-5, n
    rs = running_of(m)
    for k, v in ro.items():
        np.testing.assert_allclose(rs[k], v, rtol=1e-4, atol=1e-5, err_msg=k)
    for mo in ("rgb", "opfl"):
        assert int(getattr(m.two_fc_encoder, "visual_emb_" + mo)[1].num_batches_tracked) == 1
    return out


NAMES = list(pe.EDGE_CASES)
# input and parameter seeds of the named cases: at least one row of the greedy rollout survives its first choice (the float64
# oracle's top-1 / top-2 margins stay >= 1e-3 too, so that the rollouts are compared token for token over their whole length)
CASE_SEED = dict({n: 100 + i for i, n in enumerate(NAMES)}, k300_r64=104, c130=100)
PARAM_SEED = {"r_odd": 1025}


def _named(name):
    i = NAMES.index(name)
    dd = pe.case_dims(name)
    ragged, p = pe.case_variant(i, dd)
    d = po.make_dims(**dd)
    P = po.make_params(d, seed=PARAM_SEED.get(name, 1024))
    return d, P, po.make_running(d), po.make_inputs(d, seed=CASE_SEED[name], ragged=ragged), p, 4000 + i


@pytest.mark.parametrize("name", NAMES)
def test_named_edge_eval_vs_f64_oracle(name):
    d, P, run, x, _, _ = _named(name)
    check_eval(d, P, run, x)


@pytest.mark.parametrize("name", NAMES)
def test_named_edge_train_vs_f64_oracle(name):
    d, P, run, x, p, seed = _named(name)
    check_train(d, P, run, x, p, seed)


FUZZ = 12
FUZZ_PARAM_SEED = {9: 1025}         # (see CASE_SEED: at 1024 every row of case 9 picks EOS first)


def _fuzzed(i):
    dd = pe.fuzz_dims(i)
    ragged, p, eos = pe.fuzz_variant(i, dd)
    d = po.make_dims(**dd)
    x = po.make_inputs(d, seed=300 + i, ragged=ragged)
    return d, po.make_params(d, seed=FUZZ_PARAM_SEED.get(i, 1024), eos=eos), po.make_running(d), x, p, 5000 + i


@pytest.mark.parametrize("i", range(FUZZ))
def test_fuzzed_extents_eval_and_train_vs_f64_oracle(i):
    d, P, run, x, p, seed = _fuzzed(i)
    check_eval(d, P, run, x)
    check_train(d, P, run, x, p, seed)


# ------------------------------------------------------------------------------------------------------------------- targeted
def _one_word_batch(d, long_rows):
    """Every sentence one word except the rows of `long_rows` ({row: words})."""
    x = po.make_inputs(d, seed=9)
    T = d.L + 1
    cap = np.zeros((d.B, T), np.int64)
    cm = np.zeros((d.B, T), np.float32)
    for b in range(d.B):
        n = long_rows.get(b, 1)
        cap[b, :n] = 1 + (np.arange(n) + b) % (d.C - 1)
        cm[b, :n + 1] = 1.0
    x["cap_classes"], x["class_mask"] = cap, cm
    return x


@pytest.mark.parametrize("train", [False, True])
def test_t_prime_sees_rows_past_256(train):
    """T' is the first all-zero category column: with B = 300 only row 299 decides it."""
    d = po.make_dims(**pe.case_dims("b300"))
    assert d.B > pe.POS_TPB
    P, run = po.make_params(d), po.make_running(d)
    for words, want in ((d.L, d.L + 1), (2, 3)):
        x = _one_word_batch(d, {d.B - 1: words})
        cap_r, new_mask = po.prepare_targets(x["cap_classes"], x["class_mask"])
        o = po.forward_tf(po.to_torch(P), po.to_torch(run), *(torch.from_numpy(x[k]) for k in ("feats_rgb", "feats_opfl", "feat_mask")),
                          cap_r, new_mask)
        assert o.shape[1] == want
        if train:
            _, out = train_step(train_model(d, P, run), x)
        else:
            out = torch.from_numpy(run_model(eval_model(d, P, run), x)["tf_logp"])
        assert out.shape[1] == want, (words, out.shape)


@pytest.mark.parametrize("C", [20, 130])
def test_greedy_ties_take_lowest_index(C):
    """torch.max returns the first maximum (SAModel.py:142-166): two identical dominant rows j < k of the head -> j, in the
    one-lane-per-category head (C <= 64) and the serial head (C > 64)."""
    d = po.make_dims(B=4, K=5, R=40, A=52, E=24, C=C, L=6, F1=20, F2=12)
    P, run = po.make_params(d), po.make_running(d)
    j, k = 3, C - 2
    P["logit.weight"] = P["logit.weight"].copy()
    P["logit.bias"] = P["logit.bias"].copy()
    P["logit.weight"][k] = P["logit.weight"][j]
    P["logit.bias"][j] = P["logit.bias"][k] = 40.0
    x = po.make_inputs(d, seed=1)
    with torch.no_grad():
        seq = eval_model(d, P, run).sample(*(torch.from_numpy(x[k_]).cuda() for k_ in ("feats_rgb", "feats_opfl", "feat_mask")),
                                           {"sample_max": 1})[0]
    assert seq.shape == (d.B, d.L)
    assert (seq == j).all(), seq


def test_dominant_category_past_the_first_64_vs_f64_oracle():
    """C = 130 with one category 100 nats above the rest, in the third 64-wide chunk: the train cell's log-sum-exp must take its
    maximum over every chunk (a partial maximum overflows exp), and so must the eval cell's serial head."""
    d = po.make_dims(**pe.case_dims("c130"))
    P, run = po.make_params(d), po.make_running(d)
    P["logit.bias"] = P["logit.bias"].copy()
    P["logit.bias"][128] = 100.0
    x = po.make_inputs(d, seed=5)
    check_train(d, P, run, x, 0.0, 0)
    h, _ = check_eval(d, P, run, x)
    assert (h["seq"] == 128).all()


@pytest.mark.parametrize("max_words,Tp", [(0, 1), (1, 2)])
def test_train_t_prime_one_and_two_vs_f64_oracle(max_words, Tp):
    """max_words 0: every category column after BOS is zero (T' = 1); 1: T' = 2.  The loss scores the first T' columns of the
    rolled target (docs/POS_GENERATOR.md), as the oracle's criterion does."""
    d = po.make_dims(B=4, K=5, R=24, A=40, E=18, C=5, L=6, F1=20, F2=12)
    P, run = po.make_params(d), po.make_running(d)
    x = po.make_inputs(d, seed=3, ragged=True, max_words=max_words)
    out = check_train(d, P, run, x, 0.0, 0)
    assert out.shape[1] == Tp


def test_train_shape_beyond_attention_backward_is_refused_before_anything_moves():
    """T K * 4 > 60000 bytes (K 600 at seq_length 28): the attention backward cannot run it, so the train forward refuses it
    (XgError) before the running statistics move or a gradient is added."""
    from controllable_xgating_amd import XgError
    d = po.make_dims(B=1, K=600, R=8, A=8, E=4, C=3, L=28, F1=4, F2=4)
    assert (d.L + 1) * d.K * 4 > 60000
    P, run = po.make_params(d), po.make_running(d)
    m = train_model(d, P, run)
    m.flat_grads().zero_()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    with pytest.raises(XgError):
        train_step(m, po.make_inputs(d, seed=0))
    torch.cuda.synchronize()
    assert float(m.flat_grads().abs().max()) == 0.0
    for k, v in m.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k
