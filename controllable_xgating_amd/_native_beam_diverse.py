"""ctypes binding of the captioner's diverse beam search in libxgate_hip.so (the C ABI declared in include/xgate_beam_diverse.h).
Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGDB_VERSION = 1                      # include/xgate_beam_diverse.h
XGDB_MAX_BEAM = 8


_lib = None


def lib():
    """The library with the xgdb_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption diverse beam", "xgdb_version", XGDB_VERSION, {
            "xgdb_version": (C.c_int, []),
            "xgdb_workspace_bytes": (C.c_size_t, [PD, C.c_int32, C.c_int32, C.c_int32]),
            "xgdb_beam_search": (C.c_int, [vp, PD, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, PP, PB, PX, PR, vp, vp, vp, vp,
                                           vp, C.c_size_t]),
        })
    return _lib
