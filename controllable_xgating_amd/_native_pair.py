"""ctypes binding of the SCST rollout pair under train-mode dropout in libxgate_hip.so (the C ABI declared in
include/xgate_pair.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGPR_VERSION = 1                      # include/xgate_pair.h


_lib = None


def lib():
    """The library with the xgpr_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "rollout pair", "xgpr_version", XGPR_VERSION, {
            "xgpr_version": (C.c_int, []),
            "xgpr_rollout_pair_videos": (C.c_int, [vp, PD, PP, PB, PX, PR, C.c_uint32, vp, C.c_float, vp, C.c_size_t, PD, vp,
                                                   C.c_size_t, C.c_int, vp, vp, vp]),
        })
    return _lib
