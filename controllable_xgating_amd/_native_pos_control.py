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
    if _lib is None:
        L = npos.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
        _lib = npos.declare(L, "POS control", "xgpc_version", XGPC_VERSION, {
            "xgpc_version": (C.c_int, []),
            "xgpc_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgpc_sample_forced": (C.c_int, [vp, PD, C.c_int32, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]),
        })
    return _lib
