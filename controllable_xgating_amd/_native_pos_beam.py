"""ctypes binding of the POS generator's beam-search entry points in libxgate_hip.so (the C ABI declared in
include/xgate_pos_beam.h).  Same library and conventions as _native_pos_sample.py; there is no CPU / PyTorch fallback."""
from __future__ import annotations

import ctypes as C

from . import _native as nv
from . import _native_pos as npos

XGPB_VERSION = 1                      # include/xgate_pos_beam.h
XGPB_MAX_BEAM = 8

_lib = None


def lib():
    """The library with the xgpb_* signatures declared (loaded once)."""
    global _lib
    if _lib is not None:
        return _lib
    L = npos.lib()
    need = ("xgpb_version", "xgpb_workspace_bytes", "xgpb_beam_templates")
    missing = [n for n in need if not hasattr(L, n)]
    if missing:
        raise nv.XgError("%s lacks %s: a stale build -- rebuild it with `python __graft_entry__.py --force`"
                         % (nv.LIB_PATH, ", ".join(missing)))
    vp = C.c_void_p
    PD, PP, PB = C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState)
    L.xgpb_version.restype = C.c_int
    L.xgpb_workspace_bytes.restype = C.c_size_t
    L.xgpb_workspace_bytes.argtypes = [PD, C.c_int32]
    L.xgpb_beam_templates.restype = C.c_int
    L.xgpb_beam_templates.argtypes = [vp, PD, C.c_int32, C.c_int32, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    if L.xgpb_version() != XGPB_VERSION:
        raise nv.XgError("libxgate_hip.so carries POS beam ABI %d, this binding expects %d" % (L.xgpb_version(), XGPB_VERSION))
    _lib = L
    return L
