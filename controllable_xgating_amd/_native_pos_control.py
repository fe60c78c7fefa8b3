"""ctypes binding of the POS generator's controlled-generation entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_control.h).  Same library and conventions as _native_pos.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from . import _native_pos as npos

XGPC_VERSION = 1                      # include/xgate_pos_control.h
XGPC_TEMPLATE_GROUP = 4               # templates of one video per attention workgroup

_lib = None


def lib():
    """The library with the xgpc_* signatures declared (loaded once)."""
    global _lib
    if _lib is not None:
        return _lib
    L = npos.lib()
    need = ("xgpc_version", "xgpc_workspace_bytes", "xgpc_sample_forced")
    missing = [n for n in need if not hasattr(L, n)]
    if missing:
        raise nv.XgError("%s lacks %s: a stale build -- rebuild it with `python __graft_entry__.py --force`"
                         % (nv.LIB_PATH, ", ".join(missing)))
    vp = C.c_void_p
    PD, PP, PB = C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
    L.xgpc_version.restype = C.c_int
    L.xgpc_workspace_bytes.restype = C.c_size_t
    L.xgpc_workspace_bytes.argtypes = [PD, C.c_int32]
    L.xgpc_sample_forced.restype = C.c_int
    L.xgpc_sample_forced.argtypes = [vp, PD, C.c_int32, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    if L.xgpc_version() != XGPC_VERSION:
        raise nv.XgError("libxgate_hip.so carries POS control ABI %d, this binding expects %d" % (L.xgpc_version(), XGPC_VERSION))
    _lib = L
    return L
