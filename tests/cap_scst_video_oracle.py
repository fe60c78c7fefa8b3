"""The oracle of self-critical training on S rollouts per video (include/xgate_scst_video.h; test infrastructure): the pieces of
oracle.xgate_oracle composed the way SAModel.rollout_per_video is defined --

    encoder_fwd, init_hidden and v2a on the B videos; V, v2a(V) and the initial state repeated to the M = B S rows; the loop of
    xo.sample on the M rows, drawing from the uniforms (mode "sample") or replaying given tokens (mode "replay")

-- with ONE dropout seed: the encoder's sites then draw by element index in the B-video tensors and the decoder's by row in the M-row
tensors.  Also a numpy reference of the three advantage rules and of the criterion, the cases of tests/test_gpu_cap_scst_video.py,
their inputs (made once, never changed) and what each case reaches."""
import functools

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG

GROUP = 4            # csrc/xg_kernels.h: XGK_ATTN_BWD_GROUP = XGCC_TEMPLATE_GROUP, rows of one video per workgroup of the fast forms
SELECT_MAX_ROWS = 128  # csrc/xg_model.hip rollout_impl: up to this many rows the vocabulary product leaves tile statistics

# name -> (CFG entry, overrides of its dims, S)
CASES = {
    "tiny_s5": ("tiny", {}, 5),                  # LDS-staged step; full-logits choice; a full group plus a partial one
    "mid_b3_s5": ("mid", dict(B=3), 5),          # packed step; tile statistics; the choice inside the step; the dropout case
    "odd_s2": ("odd", {}, 2),                    # generic step; the rows form of the attention backward
    "one_s3": ("one", {}, 3),                    # K = 1, L = 1: one core step, a one-step backward
    "rows_132": ("mid", dict(B=4), 33),          # more than 128 rows on the packed step: full-logits choice; rows that end at the first word
    "c1_s4": ("c1", dict(B=2, L=8), 4),          # the real layer sizes
    "c5_s2": ("c5", dict(B=2), 2),               # K 40, R 1024: the group backward's second rounds
    "mid_s1": ("mid", dict(B=4), 1),             # S = 1, compared against sample() + RewardCriterion
}
MULTI_ROW = [k for k, v in CASES.items() if v[2] > 1]
END_AT_FIRST_WORD = {"rows_132": (3, 40, 131)}   # rows whose first draw has the uniform 0: token 0, the row ends there


def cfg_of(name):
    cfg, over, _ = CASES[name]
    return dict(CFG[cfg], **over)


def dims(name):
    return pg.make_dims(**cfg_of(name)), CASES[name][2]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(d, S, P, xv, pos, u): d with d.B = videos, the parameters, the videos' inputs (feats_rgb, feats_opfl, feat_mask), the rows'
    pos_feats (M,R), row b S + s, and the uniforms (L + 1, M) float32.  numpy, never changed."""
    d, S = dims(name)
    M = d.B * S
    P = pg.make_params(d)
    v = pg.make_inputs(d, seed=0, ragged=True)
    r = pg.make_inputs(d._replace(B=M), seed=1, ragged=True)
    xv = {k: v[k] for k in ("feats_rgb", "feats_opfl", "feat_mask")}
    u = np.random.default_rng(11).random((d.L + 1, M)).astype(np.float32)
    for row in END_AT_FIRST_WORD.get(name, ()):
        u[1, row] = 0.0
    return d, S, P, xv, r["pos_feats"].copy(), u


def oracle_inputs(name):
    """The dict run_oracle / oracle_f64_with_flips take: the videos' inputs and the rows' pos_feats."""
    _, _, _, xv, pos, _ = case_inputs(name)
    return dict(xv, pos_feats=pos)


def repeated_inputs(name):
    """The same batch with every video repeated S times: what sample() / xo.sample take."""
    d, S, P, xv, pos, u = case_inputs(name)
    x = {k: np.repeat(a, S, axis=0) for k, a in xv.items()}
    x["pos_feats"] = pos
    return d._replace(B=d.B * S), P, x, u


def composed_sample(P, feats_rgb, feats_opfl, feat_mask, pos_rows, S, L, mode="sample", uniforms=None, forced=None, temperature=1.0,
                    train=True, p=0.0, seed=0, running=None, return_logp=False, relu_trace=None):
    """The composition of the module docstring: xo.sample's loop (oracle/xgate_oracle.py: sample) on the M rows behind the videos'
    encoder.  P and the inputs are torch tensors.  Returns seq (M,n) int64, seqLogprobs (M,n) (differentiable) and, optionally,
    the per-step log-probs."""
    V = xo.encoder_fwd(P, feats_rgb, feats_opfl, feat_mask, train, p, seed, running, relu_trace=relu_trace)
    state = xo.init_hidden(P, V, feat_mask)
    vproj = xo._lin(V, P, "lstmcore.v2a")
    rep = lambda t: t.repeat_interleave(S, dim=0)      # noqa: E731
    V, vproj = rep(V), rep(vproj)
    state = [(rep(h), rep(c)) for h, c in state]
    M = V.shape[0]
    seqs, slps, logps = [], [], []
    logp = None
    unfinished = None
    for t in range(L + 1):
        if t == 0:
            it = torch.zeros(M, dtype=torch.int64)
        else:
            if mode == "replay":
                if t - 1 >= forced.shape[1]:
                    break
                it = forced[:, t - 1].clone()
            else:
                lp = logp.detach().numpy()
                it = torch.tensor([xo.sample_token(lp[b], float(uniforms[t, b]), temperature) for b in range(M)], dtype=torch.int64)
            slp = logp.gather(1, it.unsqueeze(1)).squeeze(1)
        xt = P["embed.weight"][it]
        fed = it
        if t >= 1:
            unfinished = (it > 0) if t == 1 else unfinished & (it > 0)
            if mode != "replay" and int(unfinished.sum()) == 0:
                break
            if mode != "replay":
                it = it * unfinished.to(it.dtype)
            seqs.append(it)
            slps.append(slp)
        mk = torch.ones(M, 1) if t == 0 else unfinished.to(V.dtype).unsqueeze(1)
        out, state, _ = xo.core_step(P, xt, mk, V, pos_rows, state, p, seed, t, train, vproj, relu_trace, fed)
        logp = torch.log_softmax(xo._rpoint(xo._lin(out, P, "logit"), "logit.out"), dim=1)
        logps.append(logp)
    if not seqs:
        res = (torch.zeros(M, 0, dtype=torch.int64), torch.zeros(M, 0))
    else:
        res = (torch.stack(seqs, 1), torch.stack(slps, 1))
    return res + (logps,) if return_logp else res


def draw(name, train=True, p=0.0, seed=0, temperature=1.0, dtype=torch.float32):
    """The composed oracle's own draw of a case from its uniforms, in `dtype`: (seq (M,n) ndarray, per-step log-probs)."""
    d, S, P, xv, pos, u = case_inputs(name)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        Pt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in P.items()}
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)      # noqa: E731
        with torch.no_grad():
            s, _, lps = composed_sample(Pt, f(xv["feats_rgb"]), f(xv["feats_opfl"]), f(xv["feat_mask"]), f(pos), S, d.L, "sample",
                                        uniforms=u, temperature=temperature, train=train, p=p, seed=seed, running=xo.new_running(d),
                                        return_logp=True)
    finally:
        torch.set_default_dtype(old)
    return s.numpy(), lps


@functools.lru_cache(maxsize=None)
def case_draw(name, train=True, p=0.0, seed=0, temperature=1.0):
    """draw() in float32 (computed once per argument set, shared, never changed)."""
    return draw(name, train, p, seed, temperature)


# ---- the criterion (numpy, float64)
def advantages(score, baseline="mean_others", base=None):
    """The three rules of include/xgate_scst_video.h on score (B,S): None, "mean_others" or "given" with base (B,)."""
    score = np.asarray(score, np.float64)
    B, S = score.shape
    if baseline is None:
        return score.copy()
    if baseline == "mean_others":
        assert S >= 2
        return score - (score.sum(1, keepdims=True) - score) / (S - 1)
    assert baseline == "given"
    return score - np.asarray(base, np.float64)[:, None]


def reward_mask(seq, n=None):
    """RewardCriterion's mask on seq (..., L): column 0, column t where word t - 1 is no end; nothing from column n on."""
    seq = np.asarray(seq)
    m = np.concatenate([np.ones(seq.shape[:-1] + (1,), bool), seq[..., :-1] > 0], -1)
    if n is not None:
        m[..., n:] = False
    return m


def criterion(slp, seq, adv, n=None):
    """(loss, dslp) of the criterion: -sum(slp adv mask) / sum(mask) over (B,S,L) and its gradient."""
    slp = np.asarray(slp, np.float64)
    m = reward_mask(seq, n)
    a = np.asarray(adv, np.float64)[..., None]
    return float((-slp * a * m).sum() / m.sum()), -a * m / m.sum()


# ---- what a case reaches (csrc/xg_model.hip: step_packed, rollout_impl; csrc/xg_train_video.hip launchers)
def packed(c):
    return c["R"] % 8 == 0 and c["E"] % 4 == 0 and c["A"] % 4 == 0


def tile_statistics(c, rows):
    """rollout_impl's fused_select for aligned operands (xg_heads.hip: xgk_vocab_select_ok); otherwise the full-logits choice."""
    return rows <= SELECT_MAX_ROWS and c["R"] % 32 == 0 and c["V"] >= 32


def choice_in_step(c, rows):
    """rollout_impl's step_select: the steps 1 .. L - 1 choose their tokens in their own first launch (80-column tiles from V 4096)."""
    return tile_statistics(c, rows) and packed(c) and -(-c["V"] // (80 if c["V"] >= 4096 else 32)) <= 256


def attn_bwd_group_form(c):
    """xgk_attn_bwd_group_form for aligned operands: the group kernel (True) or one workgroup per row (False)."""
    return c["A"] % 4 == 0 and c["R"] % 4 == 0 and 4 * GROUP * (c["R"] + (c["K"] + 3) // 4 * 4) <= 60000
