"""ctypes binding of the POS generator's diverse-beam-search entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_beam_diverse.h).  Same library and conventions as _native_pos_beam.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from . import _native_pos as npos

XGPD_VERSION = 1                      # include/xgate_pos_beam_diverse.h
XGPD_MAX_BEAM = 8


_lib = None


def lib():
    """The library with the xgpd_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = npos.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
        _lib = npos.declare(L, "diverse POS beam", "xgpd_version", XGPD_VERSION, {
            "xgpd_version": (C.c_int, []),
            "xgpd_workspace_bytes": (C.c_size_t, [PD, C.c_int32, C.c_int32]),
            "xgpd_beam_templates": (C.c_int, [vp, PD, C.c_int32, C.c_int32, C.c_float, C.c_int32, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp,
                                              vp, vp, C.c_size_t]),
        })
    return _lib
