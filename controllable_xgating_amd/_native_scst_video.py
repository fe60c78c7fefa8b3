"""ctypes binding of self-critical training on S rollouts per video in libxgate_hip.so (the C ABI declared in
include/xgate_scst_video.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGSV_VERSION = 1                      # include/xgate_scst_video.h
XGSV_BASE_NONE, XGSV_BASE_MEAN_OTHERS, XGSV_BASE_GIVEN = 0, 1, 2


_lib = None


def lib():
    """The library with the xgsv_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR, i32 = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun), C.c_int32
        _lib = declare(L, "per-video self-critical training", "xgsv_version", XGSV_VERSION, {
            "xgsv_version": (C.c_int, []),
            "xgsv_workspace_bytes": (C.c_size_t, [PD, i32]),
            "xgsv_rollout": (C.c_int, [vp, PD, i32, PP, PB, PX, PR, vp, C.c_float, vp, vp, vp, vp, C.c_size_t]),
            "xgsv_rollout_bwd": (C.c_int, [vp, PD, i32, PP, PP, PX, PR, vp, vp, C.c_size_t]),
            "xgsv_reward_fwd": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp]),
            "xgsv_reward_bwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        })
    return _lib
