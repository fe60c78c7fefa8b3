"""The workspace layout report of the diag library (xg_debug_ws_layout) and tests/ws_state.poison(), without a GPU."""
import ctypes as C
import itertools

import pytest
import torch

from controllable_xgating_amd import _native as nv
from oracle import paramgen as pg
from tests import ws_state as wss
from tests.util import CFG

SK_MAX_JOBS, XGK_SKPART_TILES = 5, 256                      # csrc/xg_kernels.h
TICKET_BYTES = SK_MAX_JOBS * (XGK_SKPART_TILES * 1024 * 2) * 4
DSTEP_SYNC_BYTES = 1024


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _dims(tag, rollout):
    """XgDims of a CFG entry for teacher forcing (T = seq.size(1) = L + 1) or a rollout (T = seq_length + 1): the two meanings
    of T in include/xgate.h coincide for the suite's inputs, so the teacher-forced case also takes a shorter batch (T = L)."""
    d = pg.make_dims(**CFG[tag])
    T = d.L + 1 if rollout else max(1, d.L)
    return wss.make_xgdims(d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H, d.F1, d.F2, T)


CASES = [(tag, rollout, mode) for tag in ("tiny", "odd", "one", "mid", "c1", "c5") for rollout in (False, True) for mode in (0, 1, 3)]


@pytest.mark.parametrize("tag,rollout,mode", CASES)
def test_layout_ranges_are_inside_disjoint_and_aligned(tag, rollout, mode):
    d = _dims(tag, rollout)
    lay = wss.layout(d, mode)
    total = nv.lib().xg_workspace_bytes_mode(C.byref(d), mode)
    assert lay.bytes == total and lay.core_bytes == nv.lib().xg_workspace_bytes_mode(C.byref(d), 0)
    assert nv.lib().xg_workspace_bytes(C.byref(d)) == nv.lib().xg_workspace_bytes_mode(C.byref(d), 1)
    ranges = dict(tickets=lay.tickets, dsync=lay.dsync, tok=lay.tok, alive=lay.alive, mirror=lay.mirror)
    for name, (a, n) in ranges.items():
        assert a % 256 == 0, name
        assert 0 <= a and a + n <= total, (name, a, n, total)
    for (na, (a, n)), (nb, (b, m)) in itertools.combinations(ranges.items(), 2):
        assert a + n <= b or b + m <= a, (na, nb)
    assert lay.tickets[1] == TICKET_BYTES and lay.dsync[1] == DSTEP_SYNC_BYTES
    assert lay.tok[1] == d.T * d.B * 8 and lay.alive[1] == 16
    assert lay.mirror[0] == lay.core_bytes
    assert lay.mirror[1] == (total - lay.core_bytes)
    assert (lay.mirror[1] > 0) == (mode == 1) and (mode != 1 or lay.mirror[1] >= lay.core_bytes // 2)
    assert lay.core_bytes % 256 == 0 and total % 256 == 0


def test_layout_refuses_bad_arguments():
    d = _dims("tiny", True)
    out = (C.c_uint64 * 12)()
    D = wss._diag_lib()
    assert D.xg_debug_ws_layout(C.byref(d), 0, None) == -1
    d.V = 1
    assert D.xg_debug_ws_layout(C.byref(d), 0, out) == -1


def test_the_product_library_does_not_export_the_layout_report():
    assert hasattr(C.CDLL(nv.LIB_DIAG_PATH), "xg_debug_ws_layout")
    assert not hasattr(C.CDLL(nv.LIB_PATH), "xg_debug_ws_layout")


@pytest.mark.parametrize("tag,rollout,mode", [("tiny", True, 0), ("tiny", False, 1), ("odd", True, 1), ("one", True, 3), ("mid", True, 1)])
def test_poison_spares_the_synchronisation_words_and_leaves_no_zero_elsewhere(tag, rollout, mode):
    d = _dims(tag, rollout)
    lay = wss.layout(d, mode)
    g = torch.Generator().manual_seed(5)
    ws = torch.randint(0, 256, (lay.bytes,), dtype=torch.uint8, generator=g)
    ws[lay.tickets[0] + 4096:lay.tickets[0] + 8192] = 0            # (and some zero words among them)
    before = ws.clone()
    assert not wss.sync_words_zero(ws, d, mode)
    wss.poison(ws, d, mode)
    keep = torch.zeros(lay.bytes, dtype=torch.bool)
    for a, n in (lay.tickets, lay.dsync):
        assert torch.equal(ws[a:a + n], before[a:a + n])
        keep[a:a + n] = True
    core = ws[:lay.core_bytes].view(torch.int32)
    special = keep[:lay.core_bytes].view(-1, 4).any(1)
    a, n = lay.tok
    special[a // 4:(a + n) // 4] = True
    assert (ws[a:a + n].view(torch.int64) == wss.POISON_TOKEN).all()
    a, n = lay.alive
    special[a // 4:(a + n) // 4] = True
    assert (ws[a:a + n].view(torch.int32) == wss.POISON_ALIVE).all()
    assert (core[~special] == wss.NAN32).all()                     # every data word of the core: a NaN, hence no zero
    assert torch.isnan(ws[:lay.core_bytes].view(torch.float32)[~special]).all()
    if lay.mirror[1]:
        mir = ws[lay.mirror[0]:lay.mirror[0] + lay.mirror[1]]
        assert (mir.view(torch.int16) == wss.NAN16).all() and torch.isnan(mir.view(torch.bfloat16).float()).all()
    z = torch.zeros(lay.bytes, dtype=torch.uint8)
    assert wss.sync_words_zero(z, d, mode)
    wss.poison(z, d, mode)
    assert wss.sync_words_zero(z, d, mode)
