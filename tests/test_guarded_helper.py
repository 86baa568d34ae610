"""CPU: tests/guarded.py catches a subtly wrong kernel.

Three fake kernels written in NumPy get what a HIP kernel gets -- raw addresses and a length --
and are each wrong in one of the ways tests/test_gpu_containment.py is there to find: a store
one 16-byte vector past the output, a store one byte before it, and a 3-tap filter that reads
x[-1] and x[n] where the row's zero padding belongs.  The canary check must fail for the first
two and the oracle comparison for the third; a correct kernel passes both.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import guarded
from guarded import guarded_input, guarded_output
from oracle import fir_oracle as fo

HQ = [1024, 2048, 1024]


def _mem(addr: int, count: int, ctype):
    """`count` elements of `ctype` at a raw address (inside a guarded allocation)."""
    return np.ctypeslib.as_array((ctype * count).from_address(addr))


def _fir3_i32(x_ptr: int, n: int, y_ptr: int, first: int = 0, last: int = 0, edges: str = "zero") -> None:
    """y[i] = round(sum_k HQ[k] x[i - k + 1]) as int32 over raw pointers; stores outputs
    [-first, n + last); edges="read" takes x[-1] and x[n] from memory instead of zeros."""
    xw = _mem(x_ptr - 2, n + 2, ctypes.c_int16).astype(np.int64)
    if edges == "zero":
        xw[0] = xw[-1] = 0
    acc = HQ[0] * xw[2:] + HQ[1] * xw[1:-1] + HQ[2] * xw[:-2]
    _mem(y_ptr, n, ctypes.c_int32)[:] = ((acc + 2048) >> 12).astype(np.int32)
    if last:  # one 16-byte vector past the end
        _mem(y_ptr + 4 * n, 4 * last, ctypes.c_int32)[:] = 7
    if first:  # bytes before the start
        _mem(y_ptr - first, first, ctypes.c_uint8)[:] = 0


@pytest.fixture(scope="module")
def case():
    x = np.random.default_rng(1).integers(-32768, 32768, 1001, dtype=np.int16)
    return x, fo.fir1d_i16_i32(x, HQ)


def _run(x, **kw):
    xg = guarded_input(torch.from_numpy(x))
    y, check = guarded_output(x.shape, torch.int32)
    _fir3_i32(xg.data_ptr(), x.size, y.data_ptr(), **kw)
    return y.numpy(), check


def test_a_correct_kernel_passes_both_checks(case):
    x, want = case
    got, check = _run(x)
    assert np.array_equal(got, want)
    check()


def test_store_one_vector_past_the_end_trips_the_canary(case):
    x, want = case
    got, check = _run(x, last=1)
    assert np.array_equal(got, want)  # the output itself is right: only the canary can tell
    with pytest.raises(AssertionError, match=rf"16 guard byte\(s\) changed; the first at byte offset {4 * x.size} "):
        check()


def test_store_one_byte_before_the_start_trips_the_canary(case):
    x, want = case
    got, check = _run(x, first=1)
    assert np.array_equal(got, want)
    with pytest.raises(AssertionError, match=r"1 guard byte\(s\) changed; the first at byte offset -1 "):
        check()


def test_reading_beside_the_input_fails_the_oracle_comparison(case):
    x, want = case
    got, check = _run(x, edges="read")
    check()  # nothing was stored outside: only the comparison can tell
    bad = np.flatnonzero(got != want)
    assert bad.tolist() == [0, x.size - 1]
    # the same kernel passes when the input merely sits in a zeroed buffer, as it does in a
    # scratch arena: the gap the hostile guards close
    buf = torch.zeros(x.size + 16, dtype=torch.int16)
    buf[8:8 + x.size] = torch.from_numpy(x)
    y = torch.empty(x.size, dtype=torch.int32)
    _fir3_i32(buf.data_ptr() + 16, x.size, y.data_ptr(), edges="read")
    assert np.array_equal(y.numpy(), want)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.float64])
def test_every_lead_gives_the_requested_alignment(dtype):
    item = torch.empty((), dtype=dtype).element_size()
    for lead in range(0, 64, item):
        a = torch.arange(37).to(dtype)
        g = guarded_input(a, lead_bytes=lead)
        y, _ = guarded_output((3, 5), dtype, lead_bytes=lead)
        for t in (g, y):
            assert t.data_ptr() % 16 == lead % 16 and t.data_ptr() % guarded.ALIGN == lead and t.is_contiguous()
        assert torch.equal(g, a)
    with pytest.raises(ValueError):
        guarded_output((4,), dtype, lead_bytes=guarded.ALIGN)
    if item > 1:
        with pytest.raises(ValueError):
            guarded_input(torch.zeros(4, dtype=dtype), lead_bytes=1)


def test_guards_hold_the_hostile_samples_and_obey_the_size_rule():
    for a, lo, hi in ((torch.zeros(100, dtype=torch.int16), -32768, 32767), (torch.zeros(100, dtype=torch.uint8), 255, 255),
                      (torch.zeros((3, 1000), dtype=torch.float64), -1e300, 1e300)):
        for lead in (0, 8):
            g = guarded_input(a, lead_bytes=lead)
            side = guarded.guard_size(a.shape, a.element_size()) // a.element_size()
            assert side * a.element_size() >= guarded.GUARD_MIN + (2 * 1000 * 8 if a.dim() == 2 else 0)
            around = _mem(g.data_ptr() - side * a.element_size(), 2 * side + a.numel(),
                          {torch.int16: ctypes.c_int16, torch.uint8: ctypes.c_uint8, torch.float64: ctypes.c_double}[a.dtype])
            assert not around[side:side + a.numel()].any()
            for band in (around[:side], around[side + a.numel():]):
                assert set(np.unique(band).tolist()) == {lo, hi}
                assert lo == hi or (band[:-1] != band[1:]).all()  # alternating
    with pytest.raises(ValueError):
        guarded.guard_size((8, 8), 1, guard_bytes=guarded.GUARD_MIN)  # 2-D: two rows more are required
    y, check = guarded_output((2, 3), torch.int32)
    assert (y.view(torch.uint8) == guarded.CANARY).all()  # the view is pre-filled too
    y.zero_()
    check()
