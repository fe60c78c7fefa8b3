"""ctypes binding of the POS generator's sampled-template entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_sample.h).  Same library and conventions as _native_pos_control.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from . import _native_pos as npos

XGPS_VERSION = 1                      # include/xgate_pos_sample.h


_lib = None


def lib():
    """The library with the xgps_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = npos.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
        _lib = npos.declare(L, "POS sampling", "xgps_version", XGPS_VERSION, {
            "xgps_version": (C.c_int, []),
            "xgps_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgps_sample_templates": (C.c_int, [vp, PD, C.c_int32, C.c_float, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                C.c_size_t]),
        })
    return _lib
