"""The oracle of the fused teacher-forced loss under scheduled sampling (include/xgate_ss.h; test infrastructure).

Plain form: xo.forward_xe with ss_prob, u_sel, u_tok (its own draw, it_trace) or forced_it (a replay of given fed tokens).  Per-video
form: the pieces of oracle.xgate_oracle composed the way SAModel.xe_loss_ss_per_video is defined --

    encoder_fwd, init_hidden and v2a on the B videos; V, v2a(V) and the initial state repeated to the M = B Q rows; forward_xe's
    loop on the M rows with its token choice; loss = lm_criterion + weight_class * cls_criterion over the M rows

-- with ONE dropout seed, as tests/cap_train_video_oracle.py composes its own.  Also the cases of tests/test_gpu_cap_ss.py, their
inputs (made once, never changed), the comparison of (T, M) token streams and what each case reaches."""
import functools

import numpy as np
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG, WEIGHT_CLASS

SELECT_MAX_ROWS = 128      # csrc/xg_heads.hip xgk_vocab_select_ok: up to this many rows the vocabulary product leaves tile statistics
GROUP = 4                  # csrc/xg_kernels.h: XGK_ATTN_BWD_GROUP
TOL_EDGE = 3e-4            # tests/util.py assert_sampled_tokens_match
MAX_EXCUSED_ROWS = 2       # the project's cap for sampled tokens

# name -> (CFG entry, overrides of its dims, Q (0: the plain form), classifier term, ss_prob, drop_prob_lm, uniform seed)
CASES = {
    "tiny": ("tiny", {}, 0, True, 0.5, 0.0, 21),                      # LDS-staged step, full-row choice
    "odd": ("odd", {}, 0, True, 0.5, 0.0, 21),                        # generic step, full-row choice
    "one": ("one", {}, 0, False, 0.5, 0.0, 21),                       # B 1, K 1, T 2: a single choice step
    "mid": ("mid", {}, 0, True, 0.5, 0.0, 21),                        # packed step, tile statistics at 32 columns, classifier targets
    "mid_p1": ("mid", {}, 0, False, 1.0, 0.0, 21),                    # every row draws at every t >= 1
    "mid_p025": ("mid", {}, 0, False, 0.25, 0.0, 21),
    "mid_edges": ("mid", {}, 0, False, 0.5, 0.0, 21),                 # u_sel == ss_prob exactly (no draw), u_tok == 0 (first column of weight)
    "mid_drop": ("mid", {}, 0, True, 0.5, 0.5, 21),                   # drop_prob_lm 0.5
    "mid_b132": ("mid", dict(B=132), 0, False, 0.5, 0.0, 21),         # more than 128 rows: full-row choice beside the packed step
    "c1_b3": ("c1", dict(B=3, L=8), 0, False, 0.5, 0.0, 21),          # 80-column tiles, real layer sizes
    "v_tiny_q3": ("tiny", {}, 3, True, 0.5, 0.0, 21),                 # partial groups
    "v_odd_q2": ("odd", {}, 2, True, 0.5, 0.0, 21),                   # rows form of the attention backward
    "v_mid_q5": ("mid", dict(B=4), 5, True, 0.5, 0.0, 21),            # group attention forward and backward
    "v_mid_q5_drop": ("mid", dict(B=4), 5, True, 0.5, 0.5, 21),       # the dropout case
    "v_mid_q33": ("mid", dict(B=4), 33, False, 0.5, 0.0, 21),         # 132 rows
    "v_c1_q4": ("c1", dict(B=2, L=8), 4, False, 0.5, 0.0, 21),        # real layer sizes
    "v_mid_q1": ("mid", dict(B=4), 1, False, 0.5, 0.0, 21),           # against xe_loss_ss on the same tokens
}
PLAIN = [k for k, v in CASES.items() if v[2] == 0]
PER_VIDEO = [k for k, v in CASES.items() if v[2] > 0]
DROP_SEED = 123457
# mid_edges: (t, m) whose u_sel is set to ss_prob exactly, and (t, m) that draw with u_tok = 0.0
EDGE_NO_DRAW = ((1, 0), (2, 5), (4, 11))
EDGE_FIRST_COLUMN = ((1, 3), (3, 7), (5, 2))


def cfg_of(name):
    return dict(CFG[CASES[name][0]], **CASES[name][1])


def rows_of(name):
    c = cfg_of(name)
    return c["B"] * max(CASES[name][2], 1)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(d, Q, P, x, u_sel, u_tok): d with d.B = videos (Q >= 1) or rows (Q == 0); x holds feats_rgb, feats_opfl, feat_mask of the
    d.B videos and pos_feats, seq, seq_mask, cap_classes, class_mask of the M rows (row b Q + q); the uniforms are (T, M) float32.
    numpy, never changed."""
    cfg, _, Q, _, ss_prob, _, useed = CASES[name]
    d = pg.make_dims(**cfg_of(name))
    M = d.B * max(Q, 1)
    P = pg.make_params(d)
    v = pg.make_inputs(d, seed=0, ragged=True)
    r = v if Q == 0 else pg.make_inputs(d._replace(B=M), seed=1, ragged=True)
    x = {k: v[k] for k in ("feats_rgb", "feats_opfl", "feat_mask")}
    x.update({k: r[k].copy() for k in ("pos_feats", "seq", "seq_mask", "cap_classes", "class_mask")})
    assert (x["seq"][:, 1:].sum(0) > 0).all()          # no step at which every row is padding (forward_xe would stop there)
    rng = np.random.default_rng(useed)
    u_sel = rng.random((d.L + 1, M)).astype(np.float32)
    u_tok = rng.random((d.L + 1, M)).astype(np.float32)
    if name == "mid_edges":
        for t, m in EDGE_NO_DRAW:
            u_sel[t, m] = np.float32(ss_prob)
        for t, m in EDGE_FIRST_COLUMN:
            u_sel[t, m] = 0.0
            u_tok[t, m] = 0.0
    return d, Q, P, x, u_sel, u_tok


def forward(P, xi, d, Q, train=True, p=0.0, seed=0, running=None, ss_prob=0.0, u_sel=None, u_tok=None, forced_it=None,
            it_trace=None, relu_trace=None):
    """(logp (M,T,V), cat (M,T,C)) of a case.  Q == 0: xo.forward_xe.  Q >= 1: the composition of the module docstring.
    P and xi are torch tensors."""
    if Q == 0:
        logp, cat, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"], xi["seq_mask"],
                                     train=train, p=p, seed=seed, running=running, ss_prob=ss_prob, u_sel=u_sel, u_tok=u_tok,
                                     forced_it=forced_it, it_trace=it_trace, relu_trace=relu_trace)
        return logp, cat
    V = xo.encoder_fwd(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], train, p, seed, running, relu_trace=relu_trace)
    state = xo.init_hidden(P, V, xi["feat_mask"])
    vproj = xo._lin(V, P, "lstmcore.v2a")
    rep = lambda t: t.repeat_interleave(Q, dim=0)      # noqa: E731
    Vr, vprojr = rep(V), rep(vproj)
    state = [(rep(h), rep(c)) for h, c in state]
    seq, mask = xi["seq"], xi["seq_mask"]
    outs, cats = [], []
    for i in range(seq.shape[1]):
        it = seq[:, i].clone()
        if forced_it is not None:
            it = forced_it[i].clone()
        elif train and i >= 1 and ss_prob > 0.0:
            lp = outs[-1].detach().numpy()
            for b in range(it.shape[0]):
                if float(u_sel[i, b]) < ss_prob:
                    it[b] = xo.sample_token(lp[b], float(u_tok[i, b]))
        if it_trace is not None:
            it_trace.append(it.clone())
        out, state, _ = xo.core_step(P, P["embed.weight"][it], mask[:, i].unsqueeze(1), Vr, xi["pos_feats"], state, p, seed, i, train,
                                     vprojr, relu_trace, it)
        logp, cat = xo.heads(P, out, p, seed, i, train, relu_trace)
        outs.append(logp)
        cats.append(cat)
    return torch.stack(outs, 1), torch.stack(cats, 1)


def losses(logp, cat, xi, cls):
    """(total, language, classifier) of xg_xe_loss_fwd."""
    lm = xo.lm_criterion(logp, xi["seq"], xi["seq_mask"])
    lc = xo.cls_criterion(cat, xi["cap_classes"], xi["seq_mask"], xi["class_mask"]) if cls else torch.zeros(())
    return lm + (WEIGHT_CLASS * lc if cls else 0.0), lm, lc


def case_seed(name):
    return DROP_SEED if CASES[name][5] > 0 else 0


def draw(name, dtype=torch.float32):
    """The oracle's own draw of a case from its uniforms, in `dtype`: (fed tokens (T, M) int64 ndarray, log-probs (M,T,V) tensor)."""
    d, Q, P, x, u_sel, u_tok = case_inputs(name)
    _, _, _, _, ss_prob, p, _ = CASES[name]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        Pt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in P.items()}
        xi = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in xo.to_torch_inputs(x).items()}
        trace = []
        with torch.no_grad():
            logp, _ = forward(Pt, xi, d, Q, True, p, case_seed(name), xo.new_running(d), ss_prob, u_sel, u_tok, it_trace=trace)
    finally:
        torch.set_default_dtype(old)
    return torch.stack(trace).numpy(), logp


@functools.lru_cache(maxsize=None)
def case_draw(name):
    """draw() in float32 (computed once, shared, never changed)."""
    return draw(name)


def replay_fn(name, fed):
    """run_oracle's fn for a case with the fed tokens `fed` (T, M) replayed: returns (loss, (lm, cls, running))."""
    d, Q = case_inputs(name)[:2]
    cls, p = CASES[name][3], CASES[name][5]
    forced = torch.from_numpy(np.ascontiguousarray(fed)).long()

    def fn(P, xi, tr):
        running = xo.new_running(d)
        logp, cat = forward(P, xi, d, Q, True, p, case_seed(name), running, forced_it=forced, relu_trace=tr)
        loss, lm, lc = losses(logp, cat, xi, cls)
        return loss, (lm.item(), lc.item(), running)

    return fn


def assert_fed_tokens_match(tok_h, tok_o, logp_o, seq, u_sel, u_tok, ss_prob, tol=TOL_EDGE, max_rows=MAX_EXCUSED_ROWS):
    """tests/util.py assert_sampled_tokens_match restated for (T, M) streams of FED tokens: `tok_h` a kernel's, `tok_o` the oracle's own
    draw with its log-probs `logp_o` (M,T,V).  Every row (column m of the streams) equal, except a row whose FIRST difference is a
    draw (u_sel < ss_prob) whose u_tok lies within `tol` of an edge of the oracle's float64 CDF interval of the token it drew; the rest
    of such a row follows other tokens and is not compared.  At most `max_rows` rows may be excused.  Returns the excused rows."""
    tok_h, tok_o = np.asarray(tok_h), np.asarray(tok_o)
    assert tok_h.shape == tok_o.shape, (tok_h.shape, tok_o.shape)
    assert np.array_equal(tok_h[0], np.asarray(seq)[:, 0])
    rows = []
    for m in np.flatnonzero((tok_h != tok_o).any(0)):
        t = int(np.flatnonzero(tok_h[:, m] != tok_o[:, m])[0])
        assert t >= 1 and float(u_sel[t, m]) < ss_prob, (m, t, int(tok_h[t, m]), int(tok_o[t, m]))      # a ground-truth token differs
        cdf = np.cumsum(np.exp(logp_o[m, t - 1].detach().double().numpy()))
        tk = int(tok_o[t, m])
        lo, hi = (cdf[tk - 1] if tk > 0 else 0.0) / cdf[-1], cdf[tk] / cdf[-1]
        uu = float(u_tok[t, m])
        assert min(abs(uu - lo), abs(uu - hi)) <= tol, (m, t, int(tok_h[t, m]), tk, lo, uu, hi)
        rows.append(int(m))
    assert len(rows) <= max_rows, rows
    return rows


# ---- what a case reaches (csrc/xg_model.hip: step_packed, ss_decoder_loop; csrc/xg_heads.hip: xgk_vocab_select_ok, xgk_ss_choice_form)
def step_form(c):
    if c["R"] % 8 == 0 and c["E"] % 4 == 0 and c["A"] % 4 == 0:
        return "packed"
    return "lds" if c["R"] % 8 == 0 else "generic"


def tile_width(c):
    return 80 if c["V"] >= 4096 else 32


def tile_statistics(c, rows):
    """ss_decoder_loop's `tiles` for aligned operands: the vocabulary product leaves tile statistics (xgk_vocab_select_ok)."""
    return rows <= SELECT_MAX_ROWS and c["R"] % 32 == 0 and c["R"] >= 32 and 32 <= c["V"] <= 32 * 4 * 256


def choice_form(c, rows):
    """xgk_ss_choice_form: "tiles" (16 lanes per row over the statistics) or "rows" (one workgroup per row over the stored logits)."""
    return "tiles" if tile_statistics(c, rows) and -(-c["V"] // tile_width(c)) <= 256 else "rows"


def attn_bwd_group_form(c):
    """xgk_attn_bwd_group_form for aligned operands: the group kernel (True) or one workgroup per row (False)."""
    return c["A"] % 4 == 0 and c["R"] % 4 == 0 and 4 * GROUP * (c["R"] + (c["K"] + 3) // 4 * 4) <= 60000
