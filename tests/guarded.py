"""Guard bands around kernel inputs and outputs -- a test helper, not a test module.

A kernel that is handed a bare pointer can be wrong in two ways no oracle comparison of its
output sees: it can store outside the output, and its result can depend on bytes outside the
input (a halo load that should have read zeros).  Both stay invisible while the tensors sit in
roomy, zero-filled or recycled allocations.  These helpers put every tensor inside ONE larger
allocation with known bytes on both sides of it:

* ``guarded_input(a)``: a contiguous view equal to ``a`` with hostile samples before and after
  it -- int16 guards alternate -32768 / 32767, uint8 guards are 255, float64 guards alternate
  -1e300 / +1e300 (other dtypes: all-ones bytes) -- so a sum that takes in one out-of-range
  sample differs from the oracle's zero padding by as much as the type allows.
* ``guarded_output(shape, dtype)``: ``(view, check)``; the whole buffer, the view included, is
  pre-filled with the canary byte (0xA5), and ``check()`` asserts on the device that every guard
  byte on both sides still holds it, reporting the first changed byte offset relative to the
  view's start (negative: before it; >= the view's size: after it).

Alignment: the view starts ``lead_bytes`` past a 512-byte boundary, so ``lead_bytes`` chooses
``data_ptr() % 16`` (and % 512) exactly.  ``lead_bytes`` must be a whole number of elements.

Guard size (a rule, not a measurement): each side is at least GUARD_MIN = 64 KiB -- more than
any vector, wave tile (4 KiB), LDS-staged row or filter halo a kernel here could overrun by --
and for tensors of two or more dimensions (frames: a 2-D kernel walks whole rows above and
below) at least two full rows of the last axis plus 64 KiB.  ``guard_bytes`` may ask for more,
never for less.

Scope: this checks the USE of out-of-range data (through the oracle comparison of the result)
and STORES into it (through the canaries).  It cannot see a load from outside the tensor whose
value is masked afterwards, nor a store that happens to write the canary value.

Safety: everything lives inside one allocation; neither helper hands out a pointer whose guard
bands are not backed by memory, so a kernel that overruns by less than a guard cannot fault.
Works on tensors of any device (the CPU included, which is how tests/test_guarded_helper.py
proves that the checks catch a wrong kernel).
"""
from __future__ import annotations

import math

import torch

GUARD_MIN = 64 * 1024
ALIGN = 512
CANARY = 0xA5

_HOSTILE = {torch.int16: (-32768, 32767), torch.uint8: (255, 255), torch.float64: (-1e300, 1e300)}


def guard_size(shape, itemsize: int, guard_bytes: int | None = None) -> int:
    """Bytes of guard on each side of a tensor of `shape`: the rule of the module docstring,
    rounded up to ALIGN."""
    need = GUARD_MIN + (2 * int(shape[-1]) * itemsize if len(shape) >= 2 else 0)
    if guard_bytes is not None:
        if guard_bytes < need:
            raise ValueError(f"guard_bytes {guard_bytes} is below the rule's minimum {need} for shape {tuple(shape)}")
        need = guard_bytes
    return (need + ALIGN - 1) // ALIGN * ALIGN


def _layout(shape, dtype, lead_bytes: int, guard_bytes, device):
    """(buffer of uint8, byte offset of the view, byte size of the view)."""
    itemsize = torch.empty((), dtype=dtype).element_size()
    if lead_bytes < 0 or lead_bytes >= ALIGN or lead_bytes % itemsize:
        raise ValueError(f"lead_bytes must be a multiple of the element size {itemsize} in [0, {ALIGN})")
    g = guard_size(shape, itemsize, guard_bytes)
    nbytes = math.prod(shape) * itemsize
    # slack of one ALIGN in front (the allocation's own alignment) and behind (the lead)
    buf = torch.empty(ALIGN + g + ALIGN + nbytes + g, dtype=torch.uint8, device=device)
    start = (-buf.data_ptr()) % ALIGN + g + lead_bytes
    assert start >= g and start + nbytes + g <= buf.numel()
    return buf, start, nbytes


def guarded_input(a: torch.Tensor, *, lead_bytes: int = 0, guard_bytes: int | None = None,
                  device=None) -> torch.Tensor:
    """A contiguous tensor equal to `a` (on `device`, default a's own) inside a larger buffer
    whose every other sample is hostile; see the module docstring."""
    device = a.device if device is None else torch.device(device)
    buf, start, nbytes = _layout(a.shape, a.dtype, lead_bytes, guard_bytes, device)
    lo, hi = _HOSTILE.get(a.dtype, (None, None))
    if lo is None:
        buf.fill_(0xFF)
    else:
        # the typed pattern is laid from the buffer's start; a lead of whole elements keeps it typed
        typed = buf[(-buf.data_ptr()) % ALIGN:]
        typed = typed[:typed.numel() // 16 * 16].view(a.dtype)
        buf.fill_(0xFF)
        typed[0::2] = lo
        typed[1::2] = hi
    view = buf[start:start + nbytes].view(a.dtype).view(a.shape)
    view.copy_(a)
    return view


def guarded_output(shape, dtype, *, lead_bytes: int = 0, guard_bytes: int | None = None, device="cpu",
                   canary: int = CANARY):
    """(view, check): an output tensor of `shape` / `dtype` pre-filled, like the whole buffer
    around it, with the canary byte; check() raises AssertionError when a guard byte changed."""
    shape = tuple(int(s) for s in shape)
    buf, start, nbytes = _layout(shape, dtype, lead_bytes, guard_bytes, torch.device(device))
    buf.fill_(canary)
    view = buf[start:start + nbytes].view(dtype).view(shape)

    def check(what: str = "output") -> None:
        for lo, hi in ((0, start), (start + nbytes, buf.numel())):
            bad = torch.nonzero(buf[lo:hi] != canary)
            if bad.numel():
                first = int(bad[0]) + lo
                raise AssertionError(
                    f"{what}: {bad.shape[0]} guard byte(s) changed; the first at byte offset {first - start} "
                    f"relative to the view (the view holds bytes [0, {nbytes})), now 0x{int(buf[first]):02x}")

    return view, check
