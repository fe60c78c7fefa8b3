"""The flip-aware gradient checker (tests/util.py: grad_misses, flip_exemptions) on the CPU: it rejects a wrong tile that the
earlier localised-difference allowance accepted, and it accepts a real flipped ReLU derivative by exempting exactly the row
that flip feeds."""
import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests.util import CFG, FLIP_SITES, ZERO_GRAD_PARAMS, flip_exemptions, grad_misses, run_oracle

W_RGB = xo.ENC + "visual_emb_rgb.0.weight"


def _old_relu_flip_rule(g, r, rtol=2e-3, atol=2e-6):
    """The allowance this checker replaced: a parameter upstream of a ReLU that missed the strict bounds passed as a
    'localised' difference when at most 1 % of its elements were outside the element-wise bound, none further than 5 % of the
    largest entry, and the cosine was at least 0.9999."""
    scale = np.abs(r).max()
    excess = np.abs(g - r) - (atol + rtol * np.abs(r) + 0.1 * rtol * scale)
    cos = float(g.ravel() @ r.ravel() / (np.linalg.norm(g) * np.linalg.norm(r)))
    return (excess > 0).mean() <= 0.01 and np.abs(g - r).max() <= atol + 5e-2 * scale and cos >= 1 - 1e-4


def test_planted_tile_fails_the_checker_and_passed_the_old_rule():
    """One wrong 32 x 32 tile (1 % of the largest entry) of the configs[1]-sized visual_emb_rgb.0.weight gradient: 0.13 % of its
    elements.  The strict bounds catch it, and so they do when other rows of the matrix are exempted; the old rule let it pass."""
    d = pg.make_dims(**CFG["c1"])
    rng = np.random.default_rng(0)
    r = rng.standard_normal((d.R, d.F1))
    g = r + 1e-6 * np.abs(r).max() * rng.standard_normal(r.shape)           # fp32-class round-off elsewhere
    assert grad_misses({W_RGB: g}, {W_RGB: r}) == []
    g[64:96, 256:288] += 0.01 * np.abs(r).max()
    assert _old_relu_flip_rule(g, r)
    bad = grad_misses({W_RGB: g}, {W_RGB: r})
    assert {b[1] for b in bad} >= {"max", "element"}, bad
    ex = np.zeros(r.shape, bool)
    ex[[3, 200, 500]] = True                                                  # exempted rows elsewhere do not hide it
    assert grad_misses({W_RGB: g}, {W_RGB: r}, exempt={W_RGB: ex}) != []


def _flip_case(site, delta):
    """Oracle XE at `mid` (train mode, p = 0) with the bias of `site` shifted so that one pre-activation, at a row that reaches
    the loss, is `delta` in float64.  Returns (loss, grads fp64, trace fp64, trace fp32, (j, token))."""
    d = pg.make_dims(**CFG["mid"])
    xn = pg.make_inputs(d, seed=0)
    Pn = pg.make_params(d)

    def fn(P, xi, tr):
        lo, _, _ = xo.forward_xe(P, xi["feats_rgb"], xi["feats_opfl"], xi["feat_mask"], xi["pos_feats"], xi["seq"],
                                 xi["seq_mask"], train=True, running=xo.new_running(d), relu_trace=tr)
        return xo.lm_criterion(lo, xi["seq"], xi["seq_mask"]), None

    _, _, _, tr = run_oracle(Pn, xn, fn, torch.float64, grad=False)
    k, b0, j = (0, 5, 7) if site == "enc.rgb" else ([t[0] for t in tr].index("pos_gate") + 2, 4, 11)
    assert tr[k][0] == site
    tok = None if tr[k][2] is None else int(tr[k][2][b0])
    bias = FLIP_SITES[site][1 if site == "enc.rgb" else 0] + ".bias"         # BatchNorm beta / the Linear's bias
    Pn = dict(Pn)
    Pn[bias] = Pn[bias].astype(np.float64).copy()
    Pn[bias][j] += delta - float(tr[k][1][b0, j])
    _, _, g64, t64 = run_oracle(Pn, xn, fn, torch.float64)
    assert abs(float(t64[k][1][b0, j]) - delta) < 1e-12
    _, _, _, t32 = run_oracle(Pn, xn, fn, torch.float32, grad=False)
    return Pn, g64, t64, t32, (j, tok)


@pytest.mark.parametrize("site", ["enc.rgb", "pos_gate"])
def test_real_flip_moves_only_its_exempted_row(site):
    """A pre-activation forced to +-1e-10 (far inside fp32 round-off of zero): the gradient with the ReLU active is the
    reference, the one with it inactive is the 'kernel'.  The flip misses the strict bounds on the parameters it feeds and only
    there; flip_exemptions finds it and exempts exactly row j of the Linear (and element j of the BatchNorm; the fed token's
    embedding row for the POS gate), after which every bound holds."""
    Pn, r, t64, t32, (j, tok) = _flip_case(site, +1e-10)
    _, g, _, _, _ = _flip_case(site, -1e-10)
    bad = grad_misses(g, r, skip=ZERO_GRAD_PARAMS)
    lin, bn = FLIP_SITES[site]
    fed = {lin + ".weight", lin + ".bias"} | ({bn + ".weight", bn + ".bias"} if bn else {"embed.weight"})
    assert bad and {b[0] for b in bad} <= fed, bad
    counts = {}
    ex = flip_exemptions(t64, t32, {k: v.shape for k, v in Pn.items()}, counts=counts)
    assert counts[site][0] >= 1
    assert ex[lin + ".weight"][j].all() and ex[lin + ".bias"][j]
    if bn:
        assert ex[bn + ".weight"][j] and ex[bn + ".bias"][j]
    else:
        assert ex["embed.weight"][tok].all()
    assert grad_misses(g, r, skip=ZERO_GRAD_PARAMS, exempt=ex) == []
    # exactly what the candidates feed: the flipped site's rows plus whatever natural candidates the run has elsewhere, each a
    # whole row / element of a parameter in FLIP_SITES (or an embedding row)
    owners = {n for s in FLIP_SITES.values() for m in s if m for n in (m + ".weight", m + ".bias")} | {"embed.weight"}
    assert set(ex) <= owners
    for name, m in ex.items():
        rows = m.reshape(m.shape[0], -1)
        assert (rows.all(1) == rows.any(1)).all(), name
        assert rows.any(1).sum() <= max(2, 0.05 * rows.shape[0]), (name, int(rows.any(1).sum()))
