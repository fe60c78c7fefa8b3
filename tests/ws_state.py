"""Test helper: which bytes of a workspace (include/xgate.h) are what, and how to fill one with garbage safely.

The byte ranges come from ``xg_debug_ws_layout`` of the diag library (csrc/xg_model.hip, -DXG_DIAG only: the same carve() as the
product library, checked below through xg_workspace_bytes{,_mode} of both).  Two ranges hold words that a kernel SPIN-WAITS on:
``tickets`` (the tagged granules of the split LSTM-backward epilogue, xg_step.hip: sk_epilogue_split) and ``dsync`` (the
counters of the diag-only dataflow step, xg_dstep.hip: wait_ctr).  No other polling loop exists under csrc/.  poison() never
writes them: a wrong value there could hang a kernel instead of giving a wrong number.  Index-typed ranges (``TOK`` int64 tokens,
``alive`` int32) get values that are wrong but valid, so a stale index a kernel reads cannot become an out-of-range address.
Everything else is fp32 data (bf16 in the mirror region) and gets a quiet NaN.
"""
import collections
import ctypes as C

import torch

from controllable_xgating_amd import _native as nv

NAN32 = 0x7FC00000          # quiet NaN, fp32
NAN16 = 0x7FC0              # quiet NaN, bf16
POISON_TOKEN = 1            # a valid vocabulary index (V > 1 always) that no rollout of the tests' models leaves everywhere
POISON_ALIVE = 0x7FFF

Layout = collections.namedtuple("Layout", "tickets dsync tok alive mirror bytes core_bytes")

_diag = None


def _diag_lib():
    global _diag
    if _diag is None:
        L = C.CDLL(nv.LIB_DIAG_PATH)
        L.xg_debug_ws_layout.restype = C.c_int
        L.xg_debug_ws_layout.argtypes = [C.POINTER(nv.XgDims), C.c_int, C.POINTER(C.c_uint64)]
        for name in ("xg_workspace_bytes", "xg_workspace_bytes_mode"):
            getattr(L, name).restype = C.c_size_t
        L.xg_workspace_bytes.argtypes = [C.POINTER(nv.XgDims)]
        L.xg_workspace_bytes_mode.argtypes = [C.POINTER(nv.XgDims), C.c_int]
        _diag = L
    return _diag


def make_xgdims(B, K, R, A, E, V, C_, H, F1, F2, T):
    d = nv.XgDims()
    d.B, d.K, d.R, d.A, d.E, d.V, d.C, d.H, d.F1, d.F2, d.T = B, K, R, A, E, V, C_, H, F1, F2, T
    return d


def layout(dims, mode):
    """Layout of a workspace of xg_workspace_bytes_mode(dims, mode) bytes: (offset, bytes) pairs + the two totals."""
    D, P = _diag_lib(), nv.lib()
    # the ranges are used on workspaces handed to the PRODUCT library: both builds must carve alike
    assert D.xg_workspace_bytes(C.byref(dims)) == P.xg_workspace_bytes(C.byref(dims))
    for m in (0, 1, 3):
        assert D.xg_workspace_bytes_mode(C.byref(dims), m) == P.xg_workspace_bytes_mode(C.byref(dims), m)
    out = (C.c_uint64 * 12)()
    rc = D.xg_debug_ws_layout(C.byref(dims), mode, out)
    assert rc == 0, rc
    v = [int(x) for x in out]
    lay = Layout((v[0], v[1]), (v[2], v[3]), (v[4], v[5]), (v[6], v[7]), (v[8], v[9]), v[10], v[11])
    assert lay.bytes == P.xg_workspace_bytes_mode(C.byref(dims), mode)
    return lay


def aligned(buf):
    """The 256-byte aligned workspace inside a pool buffer (model._ws_ptr: xg_workspace_bytes + 256 bytes of slack)."""
    off = (-buf.data_ptr()) % 256
    return buf[off:off + buf.numel() - 256]


def _fill(ws, a, n, dtype, value):
    if n:
        ws[a:a + n].view(dtype).fill_(value)


def poison(ws, dims, mode):
    """Fill a workspace (uint8 tensor, CPU or GPU, element 0 = the workspace's first byte, sized for ``mode``) with garbage:
    fp32 NaN in the core, bf16 NaN in the mirror region, valid-but-wrong integers in TOK / alive.  tickets and dsync are left
    exactly as they are."""
    lay = layout(dims, mode)
    assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() >= lay.bytes and ws.data_ptr() % 4 == 0
    special = sorted([lay.tickets, lay.dsync, lay.tok, lay.alive])
    pos = 0
    for a, n in special + [(lay.core_bytes, 0)]:
        assert a >= pos and (a - pos) % 4 == 0
        _fill(ws, pos, a - pos, torch.int32, NAN32)
        pos = a + n
    _fill(ws, lay.tok[0], lay.tok[1], torch.int64, POISON_TOKEN)
    _fill(ws, lay.alive[0], lay.alive[1], torch.int32, POISON_ALIVE)
    _fill(ws, lay.mirror[0], lay.mirror[1], torch.int16, NAN16)


def sync_words_zero(ws, dims, mode):
    """True when every word of tickets and dsync is zero (the caller synchronises the device first)."""
    lay = layout(dims, mode)
    return all(not bool(ws[a:a + n].any()) for a, n in (lay.tickets, lay.dsync))


def pool_buffers(model):
    """(XgDims, aligned workspace) of every buffer a model's pool holds."""
    out = []
    for key, bufs in list(model._pool.free.items()) + [(k, [b]) for k, b in model._pool.scratch.items()]:
        for b in bufs:
            out.append((make_xgdims(*key[0]), aligned(b)))
    return out


def poison_pool(model):
    """poison() for every workspace in model._pool.free / model._pool.scratch; returns how many."""
    bufs = pool_buffers(model)
    for d, ws in bufs:
        poison(ws, d, model._pool.gemm_mode)
    return len(bufs)


def pool_sync_words_zero(model):
    return all(sync_words_zero(ws, d, model._pool.gemm_mode) for d, ws in pool_buffers(model))
