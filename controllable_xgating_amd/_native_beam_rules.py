"""ctypes binding of the captioner's beam search under decoding rules in libxgate_hip.so (the C ABI declared in
include/xgate_beam_rules.h).  Same library, conventions and loud failure as _native.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from ._native_pos import declare

XGBR_VERSION = 1                      # include/xgate_beam_rules.h
XGBR_MAX_BAD_END = 32
XGBR_MAX_LENGTH = 512


class XgBeamRules(C.Structure):
    _fields_ = [("no_repeat_ngram", C.c_int32), ("min_length", C.c_int32), ("bad_end", C.c_void_p), ("n_bad_end", C.c_int32),
                ("length_scale", C.c_void_p)]


_lib = None


def lib():
    """The library with the xgbr_* signatures declared (loaded once)."""
    global _lib
    if _lib is None:
        L = nv.lib()
        vp, PD, PP, PB = C.c_void_p, C.POINTER(nv.XgDims), C.POINTER(nv.XgParams), C.POINTER(nv.XgBnState)
        PX, PR, PU = C.POINTER(nv.XgBatch), C.POINTER(nv.XgRun), C.POINTER(XgBeamRules)
        _lib = declare(L, "caption beam rules", "xgbr_version", XGBR_VERSION, {
            "xgbr_version": (C.c_int, []),
            "xgbr_workspace_bytes": (C.c_size_t, [PD, C.c_int32, C.c_int32]),
            "xgbr_beam_search": (C.c_int, [vp, PD, C.c_int32, C.c_int32, C.c_int32, PU, vp, vp, PP, PB, PX, PR, vp, vp, vp, vp, vp, vp,
                                           C.c_size_t]),
        })
    return _lib
