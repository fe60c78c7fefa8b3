"""ctypes binding of the captioner's beam search under S POS templates per video in libxgate_hip.so (the C ABI declared in
include/xgate_beam_control.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGBC_VERSION = 1                      # include/xgate_beam_control.h


_lib = None


def lib():
    """The library with the xgbc_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption beam control", "xgbc_version", XGBC_VERSION, {
            "xgbc_version": (C.c_int, []),
            "xgbc_workspace_bytes": (C.c_size_t, [PD, C.c_int32, C.c_int32]),
            "xgbc_beam_search": (C.c_int, [vp, PD, C.c_int32, C.c_int32, C.c_int32, PP, PB, PX, PR, vp, vp, vp, vp, vp, C.c_size_t]),
        })
    return _lib
