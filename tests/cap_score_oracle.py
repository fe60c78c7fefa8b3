"""The oracle of scoring given captions (include/xgate_score.h): oracle.xgate_oracle's teacher-forced REPLAY on the batch with each
video repeated per row, plus the counted-column rule.  Shared by tests/test_cap_score_cpu.py and tests/test_gpu_cap_score.py."""
import types

import numpy as np
import torch

from oracle import xgate_oracle as xo


def counted_columns(tokens):
    """(M,L) bool: column 0, and every column whose preceding tokens are all non-zero (the first EOS is counted)."""
    tokens = np.asarray(tokens)
    alive = np.cumprod(tokens > 0, axis=1).astype(bool)                      # alive[:, j]: tokens[:, :j + 1] all non-zero
    return np.concatenate([np.ones((tokens.shape[0], 1), bool), alive[:, :-1]], 1)


def _torch_rows(P, x, pos_rows, Q, dtype):
    Pt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in P.items()}
    rep = lambda k: torch.from_numpy(np.repeat(x[k], Q, 0)).to(dtype)          # noqa: E731
    pos = torch.from_numpy(np.ascontiguousarray(pos_rows)).to(dtype)
    running = xo.new_running(types.SimpleNamespace(R=pos.shape[1]))
    return Pt, (rep("feats_rgb"), rep("feats_opfl"), rep("feat_mask"), pos), running


def _finish(slp, tokens):
    cnt = counted_columns(tokens)
    tok_logp = np.where(cnt, slp, 0.0)
    return tok_logp, tok_logp.sum(1), cnt.sum(1).astype(np.int32)


def score_rows(P, x, pos_rows, tokens, Q, dtype=torch.float64):
    """Rows b Q + q: video b of `x` under pos_rows[b Q + q] with the caption tokens[b Q + q] (M,L) -> (tok_logp (M,L), score (M),
    count (M) int32) as float64 arrays computed in `dtype`: xo.sample(mode="replay", forced=tokens, train=False) on the repeated batch,
    kept in the counted columns."""
    tokens = np.asarray(tokens, dtype=np.int64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        Pt, inp, running = _torch_rows(P, x, pos_rows, Q, dtype)
        with torch.no_grad():
            _, slp = xo.sample(Pt, *inp, tokens.shape[1], mode="replay", forced=torch.from_numpy(tokens), train=False, running=running)
    finally:
        torch.set_default_dtype(old)
    return _finish(slp.double().numpy(), tokens)


def score_rows_xe(P, x, pos_rows, tokens, Q, dtype=torch.float64, raw_logit_max=None):
    """The same through another route of the oracle: xo.forward_xe(train=False) with seq = [BOS, tokens] and the `unfinished` mask,
    log-probs gathered at the tokens.  (forward_xe stops at a column of zeros: the columns behind it are counted for no row.)
    raw_logit_max: a list that receives the largest raw logit h2' W^T + b of all steps."""
    tokens = np.asarray(tokens, dtype=np.int64)
    M, L = tokens.shape
    seq = np.concatenate([np.zeros((M, 1), np.int64), tokens], 1)
    mask = np.concatenate([counted_columns(tokens), np.zeros((M, 1), bool)], 1)             # step i runs unmasked while the row is unfinished
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        Pt, inp, running = _torch_rows(P, x, pos_rows, Q, dtype)
        trace = []
        with torch.no_grad():
            logp, _, _ = xo.forward_xe(Pt, *inp, torch.from_numpy(seq), torch.from_numpy(mask).to(dtype), train=False, running=running,
                                       trace=trace)
            if raw_logit_max is not None:
                raw_logit_max.append(max(float((t["h2"] @ Pt["logit.weight"].T + Pt["logit.bias"]).max()) for t in trace))
    finally:
        torch.set_default_dtype(old)
    n = min(logp.shape[1], L)
    slp = np.zeros((M, L))
    slp[:, :n] = logp[:, :n].gather(2, torch.from_numpy(tokens[:, :n]).unsqueeze(2)).squeeze(2).double().numpy()
    return _finish(slp, tokens)


def edge_captions(M, L, V, seed, last_tile=32):
    """(M,L) int64 captions in [0, V), M >= 3: row 0 is EMPTY (starts with EOS), row 1 has no EOS, row 2 has its EOS in the last
    column (for L = 1 that is row 0 again, and row 2 is a second caption without EOS).  Rows 1 and 2 begin with the targets 1, V - 1
    and the first column of the last vocabulary tile of `last_tile` columns, as far as L allows (V - 1 lies in that tile too).  The
    other rows are random words with a random end behind the third column."""
    from oracle import paramgen as pg
    assert M >= 3 and L >= 1 and V >= 3
    tok = pg.randint("score_captions", (M, L), seed, 1, V).astype(np.int64)
    ends = pg.randint("score_ends", (M,), seed, min(3, L), L + 1)            # (row 0 alone is empty; three words tell two rows apart)
    for m in range(M):
        tok[m, ends[m]:] = 0
    tile0 = max(1, ((V - 1) // last_tile) * last_tile)
    tok[0] = 0
    tok[1:3] = pg.randint("score_edge", (2, L), seed, 1, V)
    for m, lead in ((1, (1, V - 1, tile0)), (2, (V - 1, tile0, 1))):
        n = min(len(lead), L if m == 1 or L == 1 else L - 1)
        tok[m, :n] = lead[:n]
    if L > 1:
        tok[2, L - 1] = 0
    return tok


# ---- the cases of the GPU test (tests/test_gpu_cap_score.py); tests/test_cap_score_cpu.py checks their preconditions without a GPU
LP_TOL = 3e-4                                                   # the project's bound on a log-probability of this model
TILE = 32                                                       # XGK_SCORE_TILE: vocabulary columns per tile statistic (the one width)
ROW_TILE = 128                                                  # rows per workgroup of the fast scoring form
CHUNK = 3                                                       # steps per chunk of the vocabulary scoring (SC_CHUNK)


def _cfg(name, **kw):
    from tests.util import CFG
    return dict(CFG[name], **kw)


# name -> (dims, Q, logit_gain): the smallest shapes that reach each branch
def cases():
    return {
        "tiny_q3": (_cfg("tiny"), 3, 8.0),                      # 15 rows, Q below the attention group
        "tiny_q5": (_cfg("tiny"), 5, 8.0),                      # a full attention group plus a partial one of 1
        "tiny_q9": (_cfg("tiny"), 9, 8.0),                      # two full groups plus 1
        "mid_b3_q5": (_cfg("mid", B=3), 5, 8.0),                # the packed step; 32-wide tiles, the last of 20 columns; 3 chunks
        "odd_q2": (_cfg("odd"), 2, 8.0),                        # the generic step, the generic scoring form
        "one_q3": (_cfg("one"), 3, 8.0),                        # K = 1, L = 1, V = 5: a single step, no chunk
        "rows_297": (_cfg("tiny", B=9), 33, 8.0),               # 297 rows (R = 24: the generic scoring form takes them row by row)
        "rows_297_r32": (_cfg("tiny", B=9, R=32), 33, 8.0),     # ... and with R = 32 the fast form: three row tiles, the last of 41 rows
        "c1_q8": (_cfg("c1", B=2, L=8), 8, 8.0),                # the real layer sizes
        "mid_v4100": (_cfg("mid", B=3, V=4100), 2, 8.0),        # V = 128 * 32 + 4: the last 32-wide tile holds 4 columns
        "hot": (_cfg("mid", B=3), 2, 512.0),                    # raw logits past fp32 exp overflow
    }


# the seed of a case's inputs, templates and captions: the first from 60 on at which the rows of every video are well apart
# (tests/test_cap_score_cpu.py: test_rows_of_one_video_are_well_apart)
SEEDS = {"tiny_q3": 60, "tiny_q5": 61, "tiny_q9": 62, "mid_b3_q5": 60, "odd_q2": 60, "one_q3": 60, "rows_297": 79, "rows_297_r32": 60,
         "c1_q8": 63, "mid_v4100": 60, "hot": 62}    # (hot: the first with a raw logit past 100)

_cache = {}


def case_inputs(name):
    """(d, Q, P, x, pos (B*Q,R), tokens (B*Q,L)) of a case; computed once, shared, never changed."""
    if name not in _cache:
        from oracle import paramgen as pg
        dd, Q, gain = cases()[name]
        d = pg.make_dims(**dd)
        seed = SEEDS[name]
        P = pg.make_params(d._replace(B=1), logit_gain=gain)
        x = pg.make_inputs(d, seed=seed, ragged=True)
        pos = pg.uniform("pos_feats_q", (d.B * Q, d.R), seed, -1.0, 1.0)
        tokens = edge_captions(d.B * Q, d.L, d.V, seed, TILE)
        _cache[name] = (d, Q, P, x, pos, tokens)
    return _cache[name]


_ref = {}


def case_reference(name, dtype=torch.float64):
    """score_rows of a case in `dtype`; computed once per (case, dtype)."""
    if (name, dtype) not in _ref:
        d, Q, P, x, pos, tokens = case_inputs(name)
        torch.set_num_threads(8)
        _ref[(name, dtype)] = score_rows(P, x, pos, tokens, Q, dtype)
    return _ref[(name, dtype)]
