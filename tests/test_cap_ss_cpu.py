"""CPU checks of the fused teacher-forced loss under scheduled sampling (include/xgate_ss.h): the oracle's own draw of every GPU case
in float32 and float64 (identical tokens: what backs the cap of two excused rows), the composed per-video oracle at Q = 1 against
xo.forward_xe, what each case holds and which launcher branch it reaches, the C ABI -- exports, C99, workspace sizes, refusals in
the documented order --, the raises of the two SAModel methods and the routing of Trainer.train_batch.  No compute on a GPU."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import paramgen as pg
from oracle import xgate_oracle as xo
from tests import cap_ss_oracle as sso
from tests import util
from tests.util import ROOT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    return ge.LIB


# ---- the oracle helper
@pytest.mark.parametrize("name", sorted(sso.CASES))
def test_oracle_draws_the_same_tokens_in_float32_and_float64(name):
    """No case needs an excuse from the oracle alone: its float32 and float64 draws feed the same token to every row at every step."""
    t32, _ = sso.case_draw(name)
    t64, _ = sso.draw(name, torch.float64)
    d, Q, _, x, u_sel, _ = sso.case_inputs(name)
    M, T = sso.rows_of(name), d.L + 1
    assert t32.shape == (T, M) and np.array_equal(t32, t64), np.argwhere(t32 != t64)
    ss_prob = sso.CASES[name][4]
    coin = u_sel < ss_prob
    coin[0] = False
    assert np.array_equal(t32[~coin], x["seq"].T[~coin])       # rows whose coin says no are fed the ground truth
    assert (t32 != x["seq"].T).any() or M * (T - 1) < 4        # ... and some drawn token differs from it


def test_composed_oracle_at_q1_equals_forward_xe():
    name = "v_mid_q1"
    d, Q, P, x, u_sel, u_tok = sso.case_inputs(name)
    ss_prob = sso.CASES[name][4]
    Pt, xi = xo.to_torch_params(P), xo.to_torch_inputs(x)
    ta, tb = [], []
    with torch.no_grad():
        la, ca = sso.forward(Pt, xi, d, 1, True, 0.0, 0, xo.new_running(d), ss_prob, u_sel, u_tok, it_trace=ta)
        lb, cb = sso.forward(Pt, xi, d, 0, True, 0.0, 0, xo.new_running(d), ss_prob, u_sel, u_tok, it_trace=tb)
    assert torch.equal(torch.stack(ta), torch.stack(tb))
    assert float((la - lb).abs().max()) <= 1e-6 and float((ca - cb).abs().max()) <= 1e-6
    assert (torch.stack(ta) != xi["seq"].t()).any()


def test_cases_hold_what_they_name():
    for name, (cfg, over, Q, cls, ss_prob, p, _) in sso.CASES.items():
        d, Q_, P, x, u_sel, u_tok = sso.case_inputs(name)
        M, T = sso.rows_of(name), d.L + 1
        assert Q_ == Q and x["feats_rgb"].shape[0] == d.B and x["seq"].shape == (M, T) and x["pos_feats"].shape == (M, d.R)
        assert u_sel.shape == u_tok.shape == (T, M) and u_sel.dtype == u_tok.dtype == np.float32
        assert (x["seq"][:, 0] == 0).all() and (x["seq_mask"][:, 0] == 1).all() and 0.0 < ss_prob <= 1.0
        if M > 1 and T > 2:
            assert (x["feat_mask"] == 0).any() or d.K == 1                                    # ragged feat_mask
            assert x["seq_mask"].sum(1).max() > x["seq_mask"].sum(1).min()                    # ragged seq_mask
    assert sso.rows_of("mid_b132") == sso.rows_of("v_mid_q33") == 132 and sso.rows_of("one") == 1 and sso.cfg_of("one")["L"] + 1 == 2
    assert sso.CASES["mid_p1"][4] == 1.0 and sso.CASES["mid_p025"][4] == 0.25
    assert sso.CASES["mid_drop"][5] == sso.CASES["v_mid_q5_drop"][5] == 0.5
    # the edge uniforms: u_sel == ss_prob exactly feeds the ground truth, u_tok == 0 the first column
    _, _, _, x, u_sel, u_tok = sso.case_inputs("mid_edges")
    tok, _ = sso.case_draw("mid_edges")
    for t, m in sso.EDGE_NO_DRAW:
        assert u_sel[t, m] == np.float32(0.5) and tok[t, m] == x["seq"][m, t]
    for t, m in sso.EDGE_FIRST_COLUMN:
        assert u_sel[t, m] < 0.5 and u_tok[t, m] == 0.0 and tok[t, m] == 0


def test_cases_reach_the_branches_they_name():
    heads = open(os.path.join(ROOT, "controllable_xgating_amd", "csrc", "xg_heads.hip")).read()
    assert re.search(r"B <= 128 && R % 32 == 0 && R >= 32 && V >= 32 && V <= 32 \* 4 \* ST", heads)      # xgk_vocab_select_ok
    assert re.search(r"a\.ntiles <= 16 \* RSW_PER", heads)                                              # xgk_ss_choice_form
    c = {k: sso.cfg_of(k) for k in sso.CASES}
    r = {k: sso.rows_of(k) for k in sso.CASES}
    form = {k: (sso.step_form(c[k]), sso.choice_form(c[k], r[k])) for k in sso.CASES}
    assert form["tiny"] == ("lds", "rows") and form["odd"] == ("generic", "rows") and form["one"] == ("packed", "rows")
    assert form["mid"] == ("packed", "tiles") and sso.tile_width(c["mid"]) == 32 and c["mid"]["V"] % 32       # a partial last tile
    assert form["mid_b132"] == ("packed", "rows") and form["v_mid_q33"] == ("packed", "rows")
    assert form["c1_b3"] == ("packed", "tiles") and sso.tile_width(c["c1_b3"]) == 80 and form["v_c1_q4"] == ("packed", "tiles")
    assert (c["c1_b3"]["R"], c["c1_b3"]["A"], c["c1_b3"]["K"], c["c1_b3"]["V"]) == (512, 1536, 26, 20000)
    assert form["v_tiny_q3"] == ("lds", "rows") and form["v_odd_q2"] == ("generic", "rows") and form["v_mid_q5"] == ("packed", "tiles")
    # rows of the tile form: not a multiple of the 16 rows of a workgroup nor of the 4 of a wave (mid 12, c1 3, v_mid_q5 20)
    assert r["mid"] % 16 and r["c1_b3"] % 4 and r["v_mid_q5"] % 16
    # the per-video backward: group form with partial groups (Q 5, 33, 3), rows form (odd)
    assert sso.attn_bwd_group_form(c["v_mid_q5"]) and sso.CASES["v_mid_q5"][2] % sso.GROUP and sso.CASES["v_tiny_q3"][2] % sso.GROUP
    assert not sso.attn_bwd_group_form(c["v_odd_q2"])


# ---- the C ABI
def _header():
    txt = open(os.path.join(ROOT, "include", "xgate_ss.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declarations_equal_library_exports(built):
    syms = sorted(set(re.findall(r"\b(xgss_[a-z_0-9]+)\s*\(", _header())))
    assert syms == ["xgss_version", "xgss_workspace_bytes", "xgss_xe_loss_bwd", "xgss_xe_loss_fwd"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(xgss_[a-z_0-9]+)\b", out))) == syms
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "xgate_ss.h":
            assert not re.search(r"xgss_", open(os.path.join(ROOT, "include", h)).read(), flags=re.I), h


def test_version_through_gcc_and_xg_abi_unchanged(built, tmp_path):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_ss as nss
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "xgate_ss.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(XgDims), sizeof(XgParams), sizeof(XgBnState), sizeof(XgBatch), '
                   'sizeof(XgRun), XGSS_VERSION, XG_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    sd, sp, sb, sx, sr, ver, xver = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ver == nss.XGSS_VERSION == nss.lib().xgss_version() == 1
    assert xver == nv.XG_VERSION
    assert (sd, sp, sb, sx, sr) == tuple(ctypes.sizeof(c) for c in (nv.XgDims, nv.XgParams, nv.XgBnState, nv.XgBatch, nv.XgRun))


def _mk(d, **kw):
    from controllable_xgating_amd import _native as nv
    v = dict(d._asdict(), **kw)
    return nv.XgDims(v["B"], v["K"], v["R"], v["A"], v["E"], v["V"], v["C"], v["H"], v["F1"], v["F2"], v["L"] + 1)


def test_workspace_sizes(built):
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_ss as nss
    from controllable_xgating_amd import _native_train_video as ntv
    L = nss.lib()
    B = ctypes.byref
    for cfg in ("mid", "tiny", "odd", "c1"):
        d = pg.make_dims(**util.CFG[cfg])
        assert L.xgss_workspace_bytes(B(_mk(d)), 0) == nv.lib().xg_workspace_bytes_mode(B(_mk(d)), 0) > 0     # the plain form: a standard workspace
    d = pg.make_dims(**util.CFG["mid"])
    assert L.xgss_workspace_bytes(B(_mk(d)), -1) == 0 and L.xgss_workspace_bytes(None, 3) == 0
    for bad in (_mk(d, B=0), _mk(d, R=0), _mk(d, V=1), _mk(d, K=0)):
        assert L.xgss_workspace_bytes(B(bad), 3) == 0 and L.xgss_workspace_bytes(B(bad), 0) == 0
    assert L.xgss_workspace_bytes(B(_mk(d, L=0)), 3) == 0
    assert L.xgss_workspace_bytes(B(_mk(d, B=1 << 10)), (1 << 10) + 1) == 0 and L.xgss_workspace_bytes(B(_mk(d, B=(1 << 20) + 1)), 0) == 0
    c1 = pg.make_dims(**dict(util.CFG["c1"], B=32))
    T = c1.L + 1
    w = {Q: L.xgss_workspace_bytes(B(_mk(c1)), Q) for Q in (1, 2, 3, 4, 6, 8)}
    tv = {Q: ntv.lib().xgtv_workspace_bytes(B(_mk(c1)), Q) for Q in w}
    # the per-video form: the teacher-forced per-video workspace plus, per row, T fed tokens and the tile statistics of one step
    for Q in w:
        extra = w[Q] - tv[Q]
        per_row = 8 * T + 16 * ((c1.V + 31) // 32 + 16)
        assert 0 <= extra - 32 * Q * per_row <= 768, (Q, extra)        # (the padding of the two blocks' 256-byte alignment)
    # linear in Q: equal steps between even Q (every block of the row part is then a multiple of its 256-byte alignment)
    step = w[4] - w[2]
    assert step > 0 and w[6] - w[4] == step and w[8] - w[6] == step
    assert w[1] < w[2] < w[3] < w[4] and abs(2 * (w[3] - w[2]) - step) <= 1024 and abs(2 * (w[2] - w[1]) - step) <= 1024
    assert w[4] < nv.lib().xg_workspace_bytes_mode(B(_mk(c1, B=32 * 4)), 0)


def test_bad_arguments_return_error_codes_in_the_documented_order_without_a_gpu(built):
    """Bad dims (Q among them) or a NULL workspace -1; a workspace that is too small -4, whatever else is wrong with the call; then a
    misaligned workspace, a null pointer, ss_prob outside [0, 1] or a gemm_mode other than 0: -1.  Every pointer is a fake that is
    never dereferenced: nothing is enqueued."""
    from controllable_xgating_amd import _native as nv
    from controllable_xgating_amd import _native_ss as nss
    L = nss.lib()
    d = pg.make_dims(**util.CFG["mid"])
    B = ctypes.byref
    dims = _mk(d)
    fake = 0x7F0000000000
    P = nv.XgParams(*([fake] * len(nv.PARAM_NAMES)))
    bn = nv.XgBnState(fake, fake, fake, fake)
    big = 1 << 40

    def batch(**kw):
        v = dict(feats_rgb=fake, feats_opfl=fake, feat_mask=fake, pos_feats=fake, seq=fake, seq_mask=fake)
        v.update(kw)
        return nv.XgBatch(**v)

    def run(**kw):
        r = nv.XgRun()
        r.bn_momentum, r.bn_eps, r.train = 0.1, 1e-5, 1
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def ref(o):
        return None if o is None or o is False else B(o)

    def fwd(dm=dims, Q=3, p=P, b=bn, x=None, r=None, out=fake, tok=fake, ws=fake, nbytes=big, ss=0.5, us=fake, ut=fake, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgss_xe_loss_fwd(None, ref(dm), Q, ref(p), ref(b), ref(x), None, None, 0.0, ss, us, ut, ref(r), ws, nbytes, out, tok)

    def bwd(dm=dims, Q=3, p=P, g=P, x=None, r=None, out=fake, ws=fake, nbytes=big, **_):
        x = batch() if x is None else x
        r = run() if r is None else r
        return L.xgss_xe_loss_bwd(None, ref(dm), Q, ref(p), ref(g), ref(x), None, None, 0.0, out, ref(r), ws, nbytes)

    first = (dict(Q=-1), dict(Q=-2), dict(dm=None), dict(dm=_mk(d, B=0)), dict(dm=_mk(d, V=1)), dict(dm=_mk(d, L=0)),
             dict(dm=_mk(d, B=1 << 10), Q=(1 << 10) + 1), dict(dm=_mk(d, B=(1 << 20) + 1), Q=0), dict(ws=None))
    later = [dict(p=None), dict(x=False), dict(r=False), dict(r=run(gemm_mode=1)), dict(r=run(gemm_mode=3)), dict(ws=fake + 16), dict(out=None)]
    later += [dict(x=batch(**{k: None})) for k in ("feats_rgb", "feats_opfl", "feat_mask", "pos_feats", "seq", "seq_mask")]
    own_fwd = [dict(r=run(train=0), b=None), dict(r=run(train=0), b=nv.XgBnState(fake, None, fake, fake)), dict(tok=None),
               dict(us=None), dict(ut=None), dict(ss=-0.01), dict(ss=1.01), dict(ss=float("nan"))]
    for Q in (3, 0):
        need = L.xgss_workspace_bytes(B(dims), Q)
        for call, own in ((fwd, own_fwd), (bwd, [dict(g=None)])):
            for kw in first:                              # 1. -1, also with a workspace that is too small
                assert call(**kw) == -1 and call(**dict(kw, nbytes=8)) == -1, (call.__name__, kw)
            assert call(Q=Q, nbytes=8) == -4 and call(Q=Q, nbytes=need - 1) == -4            # 2. too small: -4, whatever else is wrong behind it
            for kw in later + own:
                assert call(**dict(kw, Q=Q, nbytes=8)) == -4, (call.__name__, kw)
            for kw in later + own:                        # 3. everything else: -1
                assert call(**dict(kw, Q=Q)) == -1, (call.__name__, kw)
                assert call(**dict(kw, Q=Q, nbytes=need)) == -1, (call.__name__, kw)
    assert fwd(Q=4, nbytes=L.xgss_workspace_bytes(B(dims), 3)) == -4                          # the workspace of Q = 3 does not serve Q = 4


# ---- the Python surface
def test_xe_loss_ss_raises(built):
    d = pg.make_dims(**util.CFG["tiny"])
    Q, T = 3, d.L + 1
    m = util.make_model(d, device="cpu", train=True)
    assert hasattr(type(m), "xe_loss_ss") and hasattr(type(m), "xe_loss_ss_per_video")
    x = {k: torch.from_numpy(v) for k, v in pg.make_inputs(d).items()}
    f = (x["feats_rgb"], x["feats_opfl"], x["feat_mask"])
    pos, seq, mask = torch.zeros(d.B, Q, d.R), torch.zeros(d.B, Q, T, dtype=torch.int64), torch.ones(d.B, Q, T)
    m.ss_prob = 0.25
    with pytest.raises(NotImplementedError):                # CPU tensors
        m.xe_loss_ss(*f, x["pos_feats"], x["seq"], x["seq_mask"])
    with pytest.raises(NotImplementedError):
        m.xe_loss_ss_per_video(*f, pos, seq, mask)
    for bad in (pos.reshape(d.B * Q, d.R), pos[1:], pos[:, :, 1:], pos[:, :2]):
        with pytest.raises(ValueError):
            m.xe_loss_ss_per_video(*f, bad, seq, mask)
    for bad in (seq.reshape(d.B * Q, T), seq[:, :2], seq[:, :, :1], seq.float()):
        with pytest.raises(ValueError):
            m.xe_loss_ss_per_video(*f, pos, bad, mask)
    with pytest.raises(ValueError):
        m.xe_loss_ss(*f, x["pos_feats"].unsqueeze(1), x["seq"], x["seq_mask"])
    for prec in ("bf16", "bf16x3"):
        m.precision = prec
        with pytest.raises(NotImplementedError):
            m.xe_loss_ss(*f, x["pos_feats"], x["seq"], x["seq_mask"])
        with pytest.raises(NotImplementedError):
            m.xe_loss_ss_per_video(*f, pos, seq, mask)
    m.precision = "fp32"
    # xe_loss_per_video keeps its refusal of scheduled sampling
    with pytest.raises(NotImplementedError):
        m.xe_loss_per_video(*f, pos, seq, mask)


class _Stub:
    """A model whose loss methods record their name and return a scalar with a graph."""

    def __init__(self, ss_prob, precision="fp32"):
        self.w = torch.nn.Parameter(torch.ones(1))
        self.ss_prob, self.precision, self.training, self.calls = ss_prob, precision, True, []

    def parameters(self):
        return iter([self.w])

    def _loss(self, name):
        def f(*a, **k):
            self.calls.append(name)
            return (self.w * 2.0).sum()
        return f

    def __getattr__(self, name):
        if name in ("xe_loss", "xe_loss_ss", "xe_loss_per_video", "xe_loss_ss_per_video"):
            return self._loss(name)
        raise AttributeError(name)

    def __call__(self, *a, **k):
        self.calls.append("model()")
        raise _Reached()


class _Reached(Exception):
    pass


def _route(ss_prob, cap_dims, precision="fp32", **opt_kw):
    from controllable_xgating_amd import driver
    model = _Stub(ss_prob, precision)
    opt = argparse.Namespace(learning_rate=4e-4, weight_class=0.5, overlap_update=False, learning_rate_decay_start=-1,
                             scheduled_sampling_start=-1, self_critical_after=-1, **opt_kw)
    tr = driver.Trainer.__new__(driver.Trainer)
    tr.model, tr.opt, tr.sc_flag, tr.grad_sync, tr.iteration = model, opt, False, None, 1
    tr.fused = getattr(opt, "fused_xe_loss", True)

    class _Opt:
        def zero_grad(self): pass
        def arm(self): pass
        def step(self): pass
    tr.optimizer = _Opt()
    cap = torch.zeros((2, 3, 4) if cap_dims == 3 else (2, 4), dtype=torch.int64)
    b = dict(feat1=None, feat2=None, feat_mask=None, pos_feat=None, cap=cap, cap_mask=None, cap_classes=None, class_mask=None)
    try:
        tr.train_batch(b)
    except _Reached:
        pass
    return model.calls


def test_trainer_routes_scheduled_sampling_to_the_fused_loss():
    assert _route(0.25, 2) == ["xe_loss_ss"]
    assert _route(0.25, 3) == ["xe_loss_ss_per_video"]
    assert _route(0.25, 2, fused_ss_loss=False) == ["model()"]
    assert _route(0.25, 2, precision="bf16") == ["model()"]
    assert _route(0.25, 2, fused_xe_loss=False) == ["model()"]
    assert _route(0.25, 3, fused_xe_loss=False) == ["xe_loss_ss_per_video"]      # (a per-video batch is fused at ss_prob 0 as well)
    for kw in (dict(fused_ss_loss=False), dict(precision="bf16")):
        with pytest.raises(NotImplementedError):
            _route(0.25, 3, **kw)
    # ss_prob = 0: the calls it makes today
    assert _route(0.0, 2) == ["xe_loss"] and _route(0.0, 3) == ["xe_loss_per_video"]
    assert _route(0.0, 2, fused_ss_loss=False) == ["xe_loss"] and _route(0.0, 2, fused_xe_loss=False) == ["model()"]
    assert _route(0.0, 3, fused_ss_loss=False) == ["xe_loss_per_video"]


def test_schedule_reaches_ss_prob():
    from controllable_xgating_amd.driver import ss_prob_for_epoch
    opt = argparse.Namespace(scheduled_sampling_start=3, scheduled_sampling_increase_every=5, scheduled_sampling_increase_prob=0.05,
                             scheduled_sampling_max_prob=0.25)
    assert ss_prob_for_epoch(opt, 7) == 0.0 and ss_prob_for_epoch(opt, 8) == 0.05 and ss_prob_for_epoch(opt, 40) == 0.25
