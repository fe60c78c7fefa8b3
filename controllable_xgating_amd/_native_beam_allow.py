"""ctypes binding of the captioner's beam search whose words must follow a POS template in libxgate_hip.so (the C ABI declared in
include/xgate_beam_allow.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGBA_VERSION = 1                      # include/xgate_beam_allow.h


_lib = None


def lib():
    """The library with the xgba_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption beam allow", "xgba_version", XGBA_VERSION, {
            "xgba_version": (C.c_int, []),
            "xgba_workspace_bytes": (C.c_size_t, [PD, C.c_int32, C.c_int32]),
            "xgba_beam_search": (C.c_int, [vp, PD, C.c_int32, C.c_int32, C.c_int32, vp, vp, PP, PB, PX, PR, vp, vp, vp, vp, vp,
                                           C.c_size_t]),
        })
    return _lib
