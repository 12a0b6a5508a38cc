"""Operands that do not start on a 16-byte boundary, for the tests that hand them to the device entries.

Every tensor the allocator returns is at least 256-byte aligned, so a suite that only passes such tensors runs one side of every
`pointer & 15` branch in the host wrappers and the kernels.  offset_view() puts the same values at an address that is aligned to the
element and to nothing more, inside one live allocation with `guard` elements on both sides:

  inputs    guards are NaN: a read outside the operand that reaches a result shows up in it;
  outputs   (buffers the callee writes) guards are SENTINEL, and guards_intact() asks that they are bit-identical afterwards.

Offsets: 4 and 8 bytes for fp32, 2 and 8 bytes for bf16 -- two of each, so that an `& 7` check cannot pass for an `& 15` one.
"""
import torch

SENTINEL = -12345.0             # the guard value of an fp32 output buffer (bf16 keeps 8 significant bits: see _sentinel)
OFFSETS = {torch.float32: (4, 8), torch.bfloat16: (2, 8), torch.int64: (8,), torch.int32: (4, 8)}


def _sentinel(dtype):
    """The finite guard value of an output buffer, representable in `dtype` (bf16 keeps 8 significant bits)."""
    return -12288.0 if dtype == torch.bfloat16 else SENTINEL


def offset_view(t, off, guard=64, fill=None):
    """A contiguous view of t's shape and values with data_ptr() % 16 == off, in the middle of a fresh 1-D buffer of t's dtype
    and device that keeps `guard` elements before and after the view.  fill: the guards' value -- NaN by default (an input), or
    a finite number such as SENTINEL for a buffer the callee writes (integer dtypes: a large negative index).  The buffer is
    reachable as the view's `_base` and through guards()."""
    esz = t.element_size()
    assert off % esz == 0 and 0 <= off < 16, "offset %d is not a multiple of the element size %d" % (off, esz)
    n = t.numel()
    pad = 16 // esz
    if fill is None:
        fill = float("nan") if t.dtype.is_floating_point else -(2 ** 30)
    buf = torch.full((n + 2 * guard + 2 * pad,), fill, dtype=t.dtype, device=t.device)
    start = guard + (off - (buf.data_ptr() + guard * esz)) % 16 // esz
    v = buf[start:start + n].view(t.shape)
    v.copy_(t.detach())
    assert v.is_contiguous(), "offset_view: the view is not contiguous"
    assert v.data_ptr() % 16 == off, "offset_view: data_ptr() %% 16 = %d, wanted %d" % (v.data_ptr() % 16, off)
    assert start >= guard and buf.numel() - (start + n) >= guard
    assert v.data_ptr() >= buf.data_ptr() + guard * esz
    assert v.data_ptr() + n * esz + guard * esz <= buf.data_ptr() + buf.numel() * esz
    return v


def output_view(shape, dtype, device, off, guard=64):
    """An uninitialised-looking output buffer at offset `off`: the view is filled with the sentinel as well (a callee that skips
    an element leaves it visible), its guards are the sentinel."""
    s = _sentinel(dtype)
    return offset_view(torch.full(tuple(shape), s, dtype=dtype, device=device), off, guard, fill=s)


def guards(v):
    """(before, after): the two guard regions of an offset_view, as 1-D views of its buffer."""
    buf = v._base
    assert buf is not None and buf.dim() == 1
    start = (v.data_ptr() - buf.data_ptr()) // v.element_size()
    return buf[:start], buf[start + v.numel():]


def guards_intact(v, fill=None):
    """True when both guard regions of an output view still hold the value they were created with, bit for bit."""
    fill = _sentinel(v.dtype) if fill is None else fill
    want = torch.tensor(fill, dtype=v.dtype, device=v.device)
    return all(bool((g.view(torch.int16 if v.element_size() == 2 else torch.int32) ==
                     want.view(torch.int16 if v.element_size() == 2 else torch.int32)).all()) for g in guards(v))


def offsets(dtype):
    return OFFSETS[dtype]


def as_param(v):
    """An offset view as a leaf that requires grad (Parameter data re-seated on the view keeps the view's address)."""
    return v.detach().requires_grad_(True)


def same_bits(a, b):
    """Bit equality of two tensors of one dtype and shape (NaN == NaN, -0 != +0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool((a.contiguous().view(it) == b.contiguous().view(it)).all())
