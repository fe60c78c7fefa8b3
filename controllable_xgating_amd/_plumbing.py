"""Native plumbing shared by SAModel (model.py) and PosModel (pos.py): the current stream as the C ABI takes it, the flat
parameter / gradient buffer with its pointer structs, the BatchNorm state struct and counters, and the dropout seed of a call.
Nothing here is on the hot path; everything here hands raw device pointers to the library, so it is stated once.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _native as nv


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Holder(nn.Module):
    """Bare container so parameter names nest like the reference's sub-modules."""


def bn_struct(encoder):
    """XgBnState of the running statistics of `encoder`'s two BatchNorm layers."""
    rgb, opfl = encoder.visual_emb_rgb[1], encoder.visual_emb_opfl[1]
    return nv.XgBnState(rgb.running_mean.data_ptr(), rgb.running_var.data_ptr(),
                        opfl.running_mean.data_ptr(), opfl.running_var.data_ptr())


def bump_bn(encoder, training, n=1):
    """num_batches_tracked of `encoder`'s two BatchNorm layers += n in train mode (one launch for both counters)."""
    if training:
        ts = [m.num_batches_tracked for m in (encoder.visual_emb_rgb[1], encoder.visual_emb_opfl[1])
              if m.num_batches_tracked is not None]
        if ts:
            torch._foreach_add_(ts, n)


def next_seed(model, seed=None):
    """The 32-bit seed of the dropout hash for one call: `seed` if given, else model.dropout_seed if set, else a fresh one
    from torch's initial seed and the model's call counter (model._call, bumped here and only here)."""
    if seed is None and model.dropout_seed is not None:
        seed = int(model.dropout_seed)
    if seed is None:
        model._call += 1
        seed = int(torch.initial_seed()) * 2654435761 + model._call * 40503
    return seed & 0xFFFFFFFF


class FlatParams:
    """Mixin for an nn.Module whose parameters the library reads through a struct of pointers (XgParams / XgpParams): all of
    them live in ONE flat fp32 buffer (one RCCL all-reduce, one Adam launch) with a gradient buffer of the same layout, and
    the nn.Parameters are views into it.  The module supplies ``_abi()``."""

    _flat = _gflat = None
    _offsets = ()                  # element offset of every parameter in the flat buffers, ABI order
    _slices = None                 # name -> (offset, numel)
    _ps_cache = _gs_cache = None   # pointer structs of _flat / _gflat, valid until the buffers are rebuilt
    _grad_writes = 0               # backwards that added to a gradient buffer so far (train.ClipAdam._grad_stamp)

    def _abi(self):
        """(parameter names in the C ABI's order, ctypes struct class with one pointer field per name)."""
        raise NotImplementedError

    def _refuse_host_params(self, first):
        """Raise unless the parameters are where the library can read them (`first`: the first one)."""
        if not first.is_cuda:
            raise nv.XgError("%s runs on an MI355X only: call model.cuda() first (no CPU path)" % type(self).__name__)

    def _plist(self):
        """The nn.Parameter objects in the C ABI's order (= state_dict order).  The objects themselves are stable for the
        life of the module (.cuda()/.to()/load_state_dict replace their DATA), so the walk over named_parameters() is
        done once."""
        pl = self.__dict__.get("_plist_cache")
        if pl is None:
            named = dict(self.named_parameters())
            pl = [named[n] for n in self._abi()[0]]
            self.__dict__["_plist_cache"] = pl
        return pl

    def _ensure_flat(self):
        """Move the parameters into the flat buffer (existing gradients into the gradient buffer; None stays None).
        Rebuilt if .cuda()/.to() replaced the storages."""
        plist = self._plist()
        first = plist[0]
        if self._flat is not None and self._flat.device == first.device:
            base = self._flat.data_ptr()
            if all(p.data_ptr() == base + 4 * off for p, off in zip(plist, self._offsets)):
                return
        self._refuse_host_params(first)
        total = sum((p.numel() + 63) // 64 * 64 for p in plist)
        flat = torch.zeros(total, dtype=torch.float32, device=first.device)
        gflat = torch.zeros(total, dtype=torch.float32, device=first.device)
        off = 0
        self._slices = {}
        self._offsets = []
        for n, p in zip(self._abi()[0], plist):
            if p.dtype != torch.float32:
                raise nv.XgError("fp32 parameters only")
            k = p.numel()
            v = flat[off:off + k].view_as(p)
            v.copy_(p.data)
            had_grad = p.grad is not None
            if had_grad:
                gflat[off:off + k].view_as(p).copy_(p.grad)
            p.data = v
            p.grad = gflat[off:off + k].view_as(p) if had_grad else None
            self._slices[n] = (off, k)
            self._offsets.append(off)
            off += (k + 63) // 64 * 64
        self._flat, self._gflat = flat, gflat
        self._ps_cache = None
        self._gs_cache = None

    def flat_parameters(self):
        self._ensure_flat()
        return self._flat

    def flat_grads(self):
        """Flat gradient buffer; binds every p.grad to its slice (zeroing is the caller's zero_grad)."""
        self._ensure_flat()
        base = self._gflat.data_ptr()
        for p, off in zip(self._plist(), self._offsets):
            if p.grad is None or p.grad.data_ptr() != base + 4 * off:
                v = self._gflat[off:off + p.numel()].view_as(p)
                if p.grad is not None:
                    v.copy_(p.grad)
                else:
                    v.zero_()
                p.grad = v
        return self._gflat

    def _struct_of(self, buf):
        base = buf.data_ptr()
        return self._abi()[1](*[base + 4 * off for off in self._offsets])

    def _params_struct(self):
        """Pointer struct of the flat buffer's slices (cached until the buffer is rebuilt)."""
        self._ensure_flat()
        if self._ps_cache is None:
            self._ps_cache = self._struct_of(self._flat)
        return self._ps_cache

    def _grads_bound(self):
        base = self._gflat.data_ptr()
        for p, off in zip(self._plist(), self._offsets):
            g = p.grad
            if g is None or g.data_ptr() != base + 4 * off:
                return False
        return True

    def _grads_struct(self):
        """(g, pointer struct of gradients): the library ADDS into them.  If every p.grad is already bound to the flat
        gradient buffer (flat_grads()), accumulate there directly and hand autograd nothing (g is None); otherwise g is a
        fresh zero buffer and ``_grad_views(g)`` are its views for autograd."""
        self._ensure_flat()
        self._grad_writes += 1     # a backward is about to add to the gradient buffer
        if self._grads_bound():
            if self._gs_cache is None:
                self._gs_cache = self._struct_of(self._gflat)
            return None, self._gs_cache
        g = torch.zeros_like(self._flat)
        return g, self._struct_of(g)

    def _grad_views(self, g):
        if g is None:
            return [None] * len(self._offsets)
        return [g[off:off + p.numel()].view_as(p) for p, off in zip(self._plist(), self._offsets)]
