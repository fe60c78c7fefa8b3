"""ctypes binding of the caption loss's gradient with respect to pos_feats in libxgate_hip.so (the C ABI declared in
include/xgate_joint.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGJ_VERSION = 1                       # include/xgate_joint.h
XGJ_FORM_XE, XGJ_FORM_VIDEO, XGJ_FORM_SS = 0, 1, 2


_lib = None


def lib():
    """The library with the xgj_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PX, PR = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "caption-loss gradient of pos_feats", "xgj_version", XGJ_VERSION, {
            "xgj_version": (C.c_int, []),
            "xgj_caption_dpos": (C.c_int, [vp, PD, C.c_int32, C.c_int32, PX, PR, vp, C.c_size_t, vp]),
            "xgj_last_kernel_width": (C.c_int, []),
        })
    return _lib
