"""ctypes binding of the POS generator's training entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_train.h).  Same library and conventions as _native_pos.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from . import _native_pos as npos

XGPT_VERSION = 1                      # include/xgate_pos_train.h


class XgptRun(C.Structure):
    _fields_ = [("train", C.c_int32), ("drop_p", C.c_float), ("seed", C.c_uint32), ("bn_momentum", C.c_float)]


_lib = None


def lib():
    """The library with the xgpt_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = npos.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
        PR = C.POINTER(XgptRun)
        _lib = npos.declare(L, "POS training", "xgpt_version", XGPT_VERSION, {
            "xgpt_version": (C.c_int, []),
            "xgpt_workspace_bytes": (C.c_size_t, [PD]),
            "xgpt_forward_train": (C.c_int, [vp, PD, PP, PB, PR, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]),
            "xgpt_backward": (C.c_int, [vp, PD, PP, PP, PR, vp, vp, vp, C.c_int32, vp, vp, C.c_size_t]),
        })
    return _lib
