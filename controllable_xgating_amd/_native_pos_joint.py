"""ctypes binding of the POS generator's joint-training entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_joint.h).  Same library and conventions as _native_pos_train.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native_pos as npos
from . import _native_pos_train as npt

XGPJ_VERSION = 1                      # include/xgate_pos_joint.h


_lib = None


def lib():
    """The library with the xgpj_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = npt.lib()
        vp, PD, PP, PR = C.c_void_p, C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(npt.XgptRun)
        _lib = npos.declare(L, "POS joint training", "xgpj_version", XGPJ_VERSION, {
            "xgpj_version": (C.c_int, []),
            "xgpj_final_state": (C.c_int, [vp, PD, C.c_int32, vp, C.c_size_t, vp]),
            "xgpj_backward": (C.c_int, [vp, PD, PP, PP, PR, vp, vp, vp, C.c_int32, vp, vp, C.c_size_t, vp]),
        })
    return _lib
