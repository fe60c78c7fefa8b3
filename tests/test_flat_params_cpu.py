"""The flat parameter / gradient buffer both models share (controllable_xgating_amd/_plumbing.py: FlatParams) and the dropout
seed of a call (next_seed), on a toy module with host tensors: the rebind rules are pointer arithmetic, not device work."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from controllable_xgating_amd._native import XgError
from controllable_xgating_amd._plumbing import FlatParams, next_seed

NAMES = ["a", "b.w", "c"]                    # the toy ABI's order; 5, 64 and 70 elements
OFFSETS, TOTAL = [0, 64, 128], 256           # every slice starts on a multiple of 64 floats


class ToyParams(C.Structure):
    _fields_ = [("p%d" % i, C.c_void_p) for i in range(3)]


class Refusing(FlatParams, nn.Module):
    """Registers its parameters in another order than the ABI lists them."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.c = nn.Parameter(torch.randn(7, 10, generator=g).to(dtype))
        self.a = nn.Parameter(torch.randn(5, generator=g))
        self.b = nn.Module()
        self.b.w = nn.Parameter(torch.randn(2, 32, generator=g))
        self._call = 0
        self.dropout_seed = None

    def _abi(self):
        return NAMES, ToyParams


class Toy(Refusing):
    def _refuse_host_params(self, first):
        pass


def _params(m):
    named = dict(m.named_parameters())
    return [named[n] for n in NAMES]


def _ptrs(s):
    return [s.p0, s.p1, s.p2]


def _slice_ptrs(buf):
    return [buf.data_ptr() + 4 * off for off in OFFSETS]


def test_ensure_flat_moves_the_parameters_into_one_padded_buffer():
    m = Toy()
    before = [p.detach().clone() for p in _params(m)]
    m._ensure_flat()
    flat = m.flat_parameters()
    assert flat.dtype == torch.float32 and flat.numel() == TOTAL and m._gflat.numel() == TOTAL
    assert list(m._offsets) == OFFSETS
    used = torch.zeros(TOTAL, dtype=torch.bool)
    for n, p, v, off in zip(NAMES, _params(m), before, OFFSETS):
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        assert torch.equal(p.detach(), v) and p.shape == v.shape
        assert m._slices[n] == (off, v.numel())
        used[off:off + v.numel()] = True
    assert not flat[~used].any() and int((~used).sum()) == TOTAL - 5 - 64 - 70
    assert m._plist() is m._plist() and [id(p) for p in m._plist()] == [id(p) for p in _params(m)]


def test_existing_grad_is_carried_and_none_stays_none():
    m = Toy()
    a, bw, c = _params(m)
    grad = torch.arange(64, dtype=torch.float32).reshape(2, 32)
    bw.grad = grad.clone()
    m._ensure_flat()
    assert a.grad is None and c.grad is None
    assert bw.grad.data_ptr() == m._gflat.data_ptr() + 4 * 64 and torch.equal(bw.grad, grad)
    assert torch.equal(m._gflat[64:128], grad.reshape(-1)) and not m._gflat[:64].any() and not m._gflat[128:].any()
    assert not m._grads_bound()


def test_rebuild_only_when_a_storage_was_replaced():
    m = Toy()
    a, bw, c = _params(m)
    values = [p.detach().clone() for p in (a, bw, c)]
    grad = torch.full((7, 10), 3.0)
    c.grad = grad.clone()
    flat, ps = m.flat_parameters(), m._params_struct()
    assert _ptrs(ps) == _slice_ptrs(flat) and m._params_struct() is ps
    m._ensure_flat()
    assert m.flat_parameters() is flat and m._params_struct() is ps
    bw.data = bw.data.clone()                                   # what .cuda() / .to() do to every parameter
    m._ensure_flat()
    flat2, ps2 = m._flat, m._params_struct()
    assert flat2 is not flat and ps2 is not ps and _ptrs(ps2) == _slice_ptrs(flat2)
    for p, v, off in zip((a, bw, c), values, OFFSETS):
        assert p.data_ptr() == flat2.data_ptr() + 4 * off and torch.equal(p.detach(), v)
    assert a.grad is None and bw.grad is None
    assert c.grad.data_ptr() == m._gflat.data_ptr() + 4 * 128 and torch.equal(c.grad, grad)


def test_flat_grads_binds_every_grad():
    m = Toy()
    a, bw, c = _params(m)
    m._ensure_flat()
    m._gflat.fill_(9.0)                                         # a None grad must be bound to a ZEROED slice
    loose = torch.full((5,), 2.0)
    a.grad = loose
    g = m.flat_grads()
    assert g is m._gflat and m._grads_bound()
    for p, ptr in zip((a, bw, c), _slice_ptrs(g)):
        assert p.grad.data_ptr() == ptr and p.grad.shape == p.shape
    assert torch.equal(a.grad, loose) and a.grad is not loose
    assert not bw.grad.any() and not c.grad.any()


def test_grads_struct_bound_and_unbound():
    m = Toy()
    a, bw, c = _params(m)
    m.flat_grads()
    assert m._grad_writes == 0
    g, s = m._grads_struct()
    assert g is None and _ptrs(s) == _slice_ptrs(m._gflat) and m._grad_writes == 1
    assert m._grad_views(None) == [None, None, None]
    g2, s2 = m._grads_struct()
    assert g2 is None and s2 is s and m._grad_writes == 2
    bw.grad = None
    g3, s3 = m._grads_struct()
    assert m._grad_writes == 3 and s3 is not s
    assert g3 is not m._gflat and g3.numel() == TOTAL and g3.dtype == torch.float32 and not g3.any()
    assert _ptrs(s3) == _slice_ptrs(g3)
    views = m._grad_views(g3)
    for v, p, ptr in zip(views, (a, bw, c), _slice_ptrs(g3)):
        assert v.data_ptr() == ptr and v.shape == p.shape
    g4, _ = m._grads_struct()
    assert g4 is not g3 and m._grad_writes == 4


def test_non_fp32_parameter_is_refused():
    m = Toy(dtype=torch.float64)
    with pytest.raises(XgError, match="fp32 parameters only"):
        m._ensure_flat()


def test_host_parameters_are_refused_unless_overridden():
    m = Refusing()
    with pytest.raises(XgError):
        m._ensure_flat()
    with pytest.raises(XgError):
        m.flat_grads()
    assert m._flat is None and all(p.grad is None for p in m.parameters())


def test_next_seed():
    m = Toy()
    m.dropout_seed = (1 << 40) + 12345
    assert next_seed(m) == 12345 and next_seed(m) == 12345 and m._call == 0
    assert next_seed(m, seed=(1 << 32) + 7) == 7 and m._call == 0           # an explicit seed wins over dropout_seed
    m.dropout_seed = None
    torch.manual_seed(0)
    for call in (1, 2, 3):
        assert next_seed(m) == (torch.initial_seed() * 2654435761 + call * 40503) & 0xFFFFFFFF
        assert m._call == call
    torch.manual_seed((1 << 63) + 5)                                        # a seed beyond 32 bits is masked, not refused
    assert next_seed(m) == (torch.initial_seed() * 2654435761 + 4 * 40503) & 0xFFFFFFFF
