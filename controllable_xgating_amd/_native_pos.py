"""ctypes binding of the POS generator's entry points in libxgate_hip.so (the C ABI declared in include/xgate_pos.h), and
declare(), the one helper that this binding and those of the other POS headers (_native_pos_train / _control / _sample / _beam) use.

Same library, same conventions and the same loud failure as _native.py: there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C

from . import _native as nv

XGP_VERSION = 1                       # include/xgate_pos.h


class XgpDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "R", "A", "E", "C", "F1", "F2", "T")]


_lib = None
PARAM_NAMES = None
XgpParams = None


def declare(L, what, version_fn, expected, signatures):
    """Declare one header's entry points on the loaded library: `signatures` maps every needed symbol to (restype, argtypes),
    argtypes None where the caller sets them afterwards.  Returns L.  Raises the stale-build error when a symbol is missing and
    the ABI error when `version_fn` does not return `expected`; `what` names the ABI in that text."""
    missing = [n for n in signatures if not hasattr(L, n)]
    if missing:
        raise nv.XgError("%s lacks %s: a stale build -- rebuild it with `python __graft_entry__.py --force`"
                         % (nv.LIB_PATH, ", ".join(missing)))
    for name, (restype, argtypes) in signatures.items():
        f = getattr(L, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    got = getattr(L, version_fn)()
    if got != expected:
        raise nv.XgError("libxgate_hip.so carries %s ABI %d, this binding expects %d" % (what, got, expected))
    return L


def lib():
    """The library with the xgp_* signatures declared (loaded once)."""
    global _lib, PARAM_NAMES, XgpParams
    if _lib is not None:
        return _lib
    L = nv.lib()
    vp, PD = C.c_void_p, C.POINTER(XgpDims)
    declare(L, "POS", "xgp_version", XGP_VERSION, {
        "xgp_version": (C.c_int, []),
        "xgp_param_count": (C.c_int, []),
        "xgp_param_name": (C.c_char_p, [C.c_int]),
        "xgp_param_numel": (C.c_int, [PD, C.c_int, C.POINTER(C.c_int64)]),
        "xgp_workspace_bytes": (C.c_size_t, [PD]),
        "xgp_encoder_fwd": (C.c_int, None),          # (the three calls take XgpParams, which needs xgp_param_count: set below)
        "xgp_forward_tf": (C.c_int, None),
        "xgp_sample_greedy": (C.c_int, None),
    })
    n = L.xgp_param_count()
    PARAM_NAMES = [L.xgp_param_name(i).decode() for i in range(n)]

    class _XgpParams(C.Structure):
        _fields_ = [("p%d" % i, C.c_void_p) for i in range(n)]

    XgpParams = _XgpParams
    PP, PB = C.POINTER(_XgpParams), C.POINTER(nv.XgBnState)
    L.xgp_encoder_fwd.argtypes = [vp, PD, PP, PB, vp, vp, vp, vp, vp, C.c_size_t]
    L.xgp_forward_tf.argtypes = [vp, PD, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.xgp_sample_greedy.argtypes = [vp, PD, PP, PB, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    _lib = L
    return L
