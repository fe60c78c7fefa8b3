"""ctypes binding of teacher-forced training on Q captions per video in libxgate_hip.so (the C ABI declared in
include/xgate_train_video.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGTV_VERSION = 1                      # include/xgate_train_video.h


_lib = None


def lib():
    """The library with the xgtv_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun)
        _lib = declare(L, "per-video training", "xgtv_version", XGTV_VERSION, {
            "xgtv_version": (C.c_int, []),
            "xgtv_workspace_bytes": (C.c_size_t, [PD, C.c_int32]),
            "xgtv_xe_loss_fwd": (C.c_int, [vp, PD, C.c_int32, PP, PB, PX, vp, vp, C.c_float, PR, vp, C.c_size_t, vp]),
            "xgtv_xe_loss_bwd": (C.c_int, [vp, PD, C.c_int32, PP, PP, PX, vp, vp, C.c_float, vp, PR, vp, C.c_size_t]),
            "xgtv_video_grads": (C.c_int, [vp, PD, C.c_int32, PP, vp, C.c_size_t, vp, vp]),
        })
    return _lib
