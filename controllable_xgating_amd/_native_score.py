"""ctypes binding of scoring given captions, Q caption rows per video, in libxgate_hip.so (the C ABI declared in
include/xgate_score.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGSC_VERSION = 1                      # include/xgate_score.h


_lib = None


def lib():
    """The library with the xgsc_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption score", "xgsc_version", XGSC_VERSION, {
            "xgsc_version": (C.c_int, []),
            "xgsc_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgsc_score_captions": (C.c_int, [vp, PD, C.c_int32, PP, PB, PX, PR, vp, vp, vp, vp, vp, C.c_size_t]),
        })
    return _lib
