"""ctypes binding of the captioner's truncated (top-k / nucleus) sampling rollout in libxgate_hip.so (the C ABI declared in
include/xgate_truncate.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGTR_VERSION = 1                      # include/xgate_truncate.h


_lib = None


def lib():
    """The library with the xgtr_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption truncated sampling", "xgtr_version", XGTR_VERSION, {
            "xgtr_version": (C.c_int, []),
            "xgtr_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgtr_rollout": (C.c_int, [vp, PD, C.c_int32, PP, PB, PX, PR, C.c_int32, C.c_float, vp, C.c_float, vp, vp, vp, vp, vp,
                                       vp, C.c_size_t]),
        })
    return _lib
