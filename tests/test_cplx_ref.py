"""CPU: the complex-tap FIR's reference helper (tests/cplx_ref.py) is right before anything leans on it.

``want`` (two real filters of the committed C oracle over the flattened row, the identity of the
helper's docstring) must equal ``cplx_loop`` (the contract of include/fir_hip.h as a direct loop over
unbounded Python ints) bit for bit: taps 1-12, 16, 17, 33, 64 and 65, widths 1-20, two rows,
acc_bits 8 / 16 / 24 / 31 / 32 / 40 / 64, frac_bits 1 / 12 / 31, both stages, random full-range int16
samples and taps, a -32768 in each tap part, and int32-sized taps at acc_bits = 64 where needs_wide
holds.  Every comparison is np.array_equal.
"""
from __future__ import annotations

import numpy as np
import pytest

import cplx_ref
from cplx_ref import OUT_I32, OUT_U8_SAT, as_real_taps, cplx_loop, want

TAPS = list(range(1, 13)) + [16, 17, 33, 64, 65]
# (acc_bits, frac_bits, stage)
ARITH = [(16, 12, OUT_I32), (24, 12, OUT_I32), (32, 12, OUT_I32), (32, 1, OUT_I32), (32, 31, OUT_I32), (8, 1, OUT_I32),
         (31, 12, OUT_I32), (40, 31, OUT_I32), (64, 12, OUT_I32), (64, 1, OUT_I32), (32, 12, OUT_U8_SAT),
         (40, 31, OUT_U8_SAT)]


def _same(x, hq, frac, acc, stage, what):
    a, b = want(x, hq, frac, acc, stage), cplx_loop(x, hq, frac, acc, stage)
    assert a.shape == b.shape == x.shape and a.dtype == b.dtype, what
    assert np.array_equal(a, b), (what, np.argwhere(a != b)[:4].tolist())


def test_as_real_taps_layout():
    g_re, g_im = as_real_taps([[1, 2], [3, 4], [5, 6]])  # c = 1, G = 7
    assert g_re.tolist() == [-2, 1, -4, 3, -6, 5, 0] and g_im.tolist() == [0, 1, 2, 3, 4, 5, 6]
    g_re, g_im = as_real_taps([[7, -8]])  # c = 0, G = 3
    assert g_re.tolist() == [8, 7, 0] and g_im.tolist() == [0, 7, -8]
    g_re, g_im = as_real_taps(np.zeros((4, 2)))
    assert len(g_re) == len(g_im) == 11


@pytest.mark.parametrize("L", TAPS)
def test_want_equals_the_direct_loop(L):
    rng = np.random.default_rng(100 + L)
    for width in range(1, 21):
        x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
        hq = rng.integers(-32768, 32768, (L, 2))
        for acc, frac, stage in ARITH:
            _same(x, hq, frac, acc, stage, (L, width, acc, frac, stage))


def test_extreme_samples_and_taps():
    """All -32768 samples against +-32767 / -32768 taps: both sums pass 2^31 many times over."""
    for L in (5, 33, 64):
        x = np.full((1, 2 * 70), -32768, np.int16)
        for hr, hi in ((32767, 32767), (32767, -32767), (-32768, 32767), (32767, -32768), (-32768, -32768)):
            hq = np.tile([[hr, hi]], (L, 1))
            for acc, frac, stage in ((16, 12, OUT_I32), (24, 1, OUT_I32), (31, 31, OUT_I32), (32, 12, OUT_I32),
                                     (64, 12, OUT_I32)):
                _same(x, hq, frac, acc, stage, (L, hr, hi, acc, frac))


def test_one_part_at_minus_32768():
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, (2, 2 * 19), dtype=np.int16)
    for L in (1, 4, 9):
        for part in (0, 1):
            hq = rng.integers(-2000, 2001, (L, 2))
            hq[L // 2, part] = -32768
            for acc in (16, 32, 40):
                _same(x, hq, 12, acc, OUT_I32, (L, part, acc))


def test_int32_sized_taps():
    """Taps of int32 size at acc_bits 32, 40 and 64 (the sums stay below 2^63: 9 taps)."""
    rng = np.random.default_rng(8)
    x = rng.integers(-32768, 32768, (2, 2 * 17), dtype=np.int16)
    hq = rng.integers(-(1 << 31) + 1, 1 << 31, (9, 2))
    hq[0] = [(1 << 31) - 1, -(1 << 31) + 1]
    for acc, frac in ((32, 12), (40, 20), (64, 12), (64, 40)):
        for stage in (OUT_I32, OUT_U8_SAT):
            _same(x, hq, frac, acc, stage, (acc, frac, stage))


def test_needs_wide_taps_at_acc_64():
    """2^16 + 3 taps of +-(2^31 - 1) in both parts: sum(|hr| + |hi|) * 32768 passes 2^63, so the
    library sums in 128 bits.  The samples are small (|x| <= 100), so every true sum stays far below
    2^63 and the C oracle's 64-bit sums are exact: ``want`` must still equal the unbounded loop."""
    rng = np.random.default_rng(9)
    L = (1 << 16) + 3
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert int(np.abs(hq).sum()) * 32768 >= 1 << 63
    x = rng.integers(-100, 101, (1, 2 * 12), dtype=np.int16)
    for acc, frac, stage in ((64, 30, OUT_I32), (80, 40, OUT_U8_SAT)):
        _same(x, hq, frac, acc, stage, (acc, frac, stage))


def test_empty_and_shapes():
    assert want(np.zeros((3, 0), np.int16), [[1, 2]]).shape == (3, 0)
    assert want(np.zeros((0, 8), np.int16), [[1, 2]]).shape == (0, 8)
    x = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    assert np.array_equal(want(x, [[3, -2], [1, 5]], 1), cplx_loop(x, [[3, -2], [1, 5]], 1))
    assert cplx_ref.want(x, [[4096, 0]], 12).tolist() == x.astype(np.int32).tolist()  # the identity filter
