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
    if _lib is not None:
        return _lib
    L = npos.lib()
    need = ("xgpt_version", "xgpt_workspace_bytes", "xgpt_forward_train", "xgpt_backward")
    missing = [n for n in need if not hasattr(L, n)]
    if missing:
        raise nv.XgError("%s lacks %s: a stale build -- rebuild it with `python __graft_entry__.py --force`"
                         % (nv.LIB_PATH, ", ".join(missing)))
    vp = C.c_void_p
    PD, PP, PB, PR = C.POINTER(npos.XgpDims), C.POINTER(npos.XgpParams), C.POINTER(nv.XgBnState), C.POINTER(XgptRun)
    L.xgpt_version.restype = C.c_int
    L.xgpt_workspace_bytes.restype = C.c_size_t
    L.xgpt_workspace_bytes.argtypes = [PD]
    L.xgpt_forward_train.restype = C.c_int
    L.xgpt_forward_train.argtypes = [vp, PD, PP, PB, PR, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.xgpt_backward.restype = C.c_int
    L.xgpt_backward.argtypes = [vp, PD, PP, PP, PR, vp, vp, vp, C.c_int32, vp, vp, C.c_size_t]
    if L.xgpt_version() != XGPT_VERSION:
        raise nv.XgError("libxgate_hip.so carries POS training ABI %d, this binding expects %d" % (L.xgpt_version(), XGPT_VERSION))
    _lib = L
    return L
