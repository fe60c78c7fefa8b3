"""ctypes binding of the POS generator's entry points in libxgate_hip.so (the C ABI declared in include/xgate_pos.h).

Same library, same conventions and the same loud failure as _native.py: there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

from . import _native as nv

XGP_VERSION = 1                       # include/xgate_pos.h


class XgpDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "R", "A", "E", "C", "F1", "F2", "T")]


_lib = None
PARAM_NAMES = None
XgpParams = None


def lib():
    """The library with the xgp_* signatures declared (loaded once)."""
    global _lib, PARAM_NAMES, XgpParams
    if _lib is not None:
        return _lib
    L = nv.lib()
    need = ("xgp_version", "xgp_param_count", "xgp_param_name", "xgp_param_numel", "xgp_workspace_bytes", "xgp_encoder_fwd",
            "xgp_forward_tf", "xgp_sample_greedy")
    missing = [n for n in need if not hasattr(L, n)]
    if missing:
        raise nv.XgError("%s lacks %s: a stale build -- rebuild it with `python __graft_entry__.py --force`"
                         % (nv.LIB_PATH, ", ".join(missing)))
    L.xgp_version.restype = C.c_int
    L.xgp_param_count.restype = C.c_int
    L.xgp_param_name.restype = C.c_char_p
    L.xgp_param_name.argtypes = [C.c_int]
    L.xgp_param_numel.restype = C.c_int
    L.xgp_param_numel.argtypes = [C.POINTER(XgpDims), C.c_int, C.POINTER(C.c_int64)]
    L.xgp_workspace_bytes.restype = C.c_size_t
    L.xgp_workspace_bytes.argtypes = [C.POINTER(XgpDims)]
    n = L.xgp_param_count()
    PARAM_NAMES = [L.xgp_param_name(i).decode() for i in range(n)]

    class _XgpParams(C.Structure):
        _fields_ = [("p%d" % i, C.c_void_p) for i in range(n)]

    XgpParams = _XgpParams
    vp = C.c_void_p
    PD, PP, PB = C.POINTER(XgpDims), C.POINTER(_XgpParams), C.POINTER(nv.XgBnState)
    sigs = {
        "xgp_encoder_fwd": [vp, PD, PP, PB, vp, vp, vp, vp, vp, C.c_size_t],
        "xgp_forward_tf": [vp, PD, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t],
        "xgp_sample_greedy": [vp, PD, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t],
    }
    for name, args in sigs.items():
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    if L.xgp_version() != XGP_VERSION:
        raise nv.XgError("libxgate_hip.so carries POS ABI %d, this binding expects %d" % (L.xgp_version(), XGP_VERSION))
    _lib = L
    return L
