"""ctypes binding of the fused teacher-forced loss under scheduled sampling in libxgate_hip.so (the C ABI declared in
include/xgate_ss.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGSS_VERSION = 1                      # include/xgate_ss.h


_lib = None


def lib():
    """The library with the xgss_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "scheduled-sampling loss", "xgss_version", XGSS_VERSION, {
            "xgss_version": (C.c_int, []),
            "xgss_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgss_xe_loss_fwd": (C.c_int, [vp, PD, C.c_int32, PP, PB, PX, vp, vp, C.c_float, C.c_float, vp, vp, PR, vp, C.c_size_t,
                                           vp, vp]),
            "xgss_xe_loss_bwd": (C.c_int, [vp, PD, C.c_int32, PP, PP, PX, vp, vp, C.c_float, vp, PR, vp, C.c_size_t]),
        })
    return _lib
