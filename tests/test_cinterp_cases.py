"""The interpolating complex-tap FIR's reference and predicted dispatch (tests/cinterp_cases.py),
held against the contract written as plain Python ints before any GPU test leans on them.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import cinterp_cases as ic
import cplx_ref
from cplx_ref import cplx_loop
from oracle import c_oracle


def _widths(L):
    return sorted({1, 2, max(1, L - 1), 9})


@pytest.mark.parametrize("U", range(1, 18))
def test_want_is_the_polyphase_loop_is_the_stuffed_loop(U):
    """want == want_loop == cplx_loop of the stuffed signal: every U in 1..17, taps from 1 up past 2 U
    (empty phases where taps < U, both parities of taps / 2), rows of 1, 2, taps - 1 and 9 frames."""
    rng = np.random.default_rng(U)
    for L in sorted(set(range(1, 8)) | {U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1, 3 * U + 2} - {0, -1}):
        hq = rng.integers(-32767, 32768, (L, 2))
        for width in _widths(L):
            x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
            x[0, :2] = (-32768, 32767)
            for acc, frac in ((32, 9), (24, 3)):
                loop = ic.want_loop(x, hq, U, frac, acc)
                assert loop.shape == (2, 2 * width * U) and loop.dtype == np.int32
                assert np.array_equal(loop, cplx_loop(ic.stuffed(x, U), hq, frac, acc)), (U, L, width, acc)
                assert np.array_equal(ic.want(x, hq, U, frac, acc), loop), (U, L, width, acc)


@pytest.mark.parametrize("stage", [ic.OUT_I32, ic.OUT_U8_SAT])
@pytest.mark.parametrize("acc", [24, 32, 40, 64])
def test_want_is_the_loop_at_every_stage_and_width_of_sum(acc, stage):
    rng = np.random.default_rng(100 * acc + stage)
    frac = 5 if stage == ic.OUT_U8_SAT else 9  # small enough that the u8 stage sees values inside (0, 255) too
    for U, L, width in ((2, 5, 7), (3, 8, 33), (4, 2, 5), (7, 33, 6), (16, 17, 3), (1, 4, 9)):
        x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
        hq = rng.integers(-40, 41, (L, 2)) if stage == ic.OUT_U8_SAT else rng.integers(-32767, 32768, (L, 2))
        got = ic.want(x, hq, U, frac, acc, stage)
        assert got.dtype == (np.uint8 if stage == ic.OUT_U8_SAT else np.int32)
        assert np.array_equal(got, ic.want_loop(x, hq, U, frac, acc, stage)), (U, L, width)


def test_want_loop_past_2_63():
    """Taps of +-(2^31 - 1): want_loop against cplx_loop of the stuffed signal, both unbounded ints."""
    rng = np.random.default_rng(7)
    L = 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    x = np.full((1, 2 * 6), 32767, np.int16)
    for U in (1, 2, 3):
        assert np.array_equal(ic.want_loop(x, hq, U, 40, 80), cplx_loop(ic.stuffed(x, U), hq, 40, 80))


def test_stuffed_and_identities():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, (2, 3, 2 * 11), dtype=np.int16)
    for U in (1, 2, 5):
        xu = ic.stuffed(x, U)
        assert xu.shape == (2, 3, 2 * 11 * U) and xu.dtype == np.int16
        v = xu.reshape(2, 3, 11 * U, 2)
        assert np.array_equal(v[:, :, ::U], x.reshape(2, 3, 11, 2))
        assert all(not v[:, :, k::U].any() for k in range(1, U))  # the U - 1 frames after the last one too
    hq = rng.integers(-3000, 3001, (7, 2))
    x2 = x.reshape(6, 22)
    # U = 1 is the full-rate reference itself
    for frac, acc, stage in ((12, 32, ic.OUT_I32), (6, 24, ic.OUT_U8_SAT)):
        assert np.array_equal(ic.want(x2, hq, 1, frac, acc, stage), cplx_ref.want(x2, hq, frac, acc, stage))
    # hi = 0 is the real oracle with two channels on the stuffed signal
    hr = hq.copy()
    hr[:, 1] = 0
    for U in (1, 2, 3, 16):
        for frac, acc, stage in ((12, 32, ic.OUT_I32), (6, 24, ic.OUT_U8_SAT), (20, 40, ic.OUT_I32)):
            real = c_oracle().fir1d_rows(ic.stuffed(x2, U), hr[:, 0], frac, acc, stage, channels=2)
            assert np.array_equal(ic.want(x2, hr, U, frac, acc, stage), real), (U, frac, acc, stage)


def test_window_buckets_and_shape_lists():
    for U in range(2, 17):
        for L in range(1, ic.fast_max_taps(U) + 1):
            w, per = ic.window(L, U), -(-L // U)
            assert per <= w <= per + 1 or (L < U and w == 1), (L, U, w)
            assert ic.bucket(L, U) >= w and ic.bucket(L, U) in ic.BUCKETS
        assert max(ic.window(L, U) for L in range(1, ic.fast_max_taps(U) + 1)) <= ic.BUCKETS[-1]
    # where U divides taps and taps / 2, every phase has the same centre: no extra window frame
    assert ic.window(64, 4) == 16 and ic.window(128, 8) == 16 and ic.window(32, 2) == 16 and ic.window(16, 16) == 2
    assert [ic.window(5 * U, U) for U in (2, 4, 8)] == [6, 6, 6]
    assert [ic.tile(U) for U in (2, 3, 4, 5, 8, 16)] == [1024, 512, 512, 256, 256, 256]
    for U in (2, 3, 4, 8, 16):
        T = ic.tile(U)
        assert ic.F % T == 0 and (T * U * 8 <= 16384 or T == 256)
        edges = ic.edge_widths(U)
        for mark in (1, ic.W, ic.PASS, T, ic.F, 2 * ic.F):
            assert {mark, mark + 1} <= set(edges) and (mark == 1 or mark - 1 in edges)
        assert max(edges) == 2 * ic.F + 1
        assert all(w % ic.ROW_UNIT == 0 for _, w in ic.multi_row_shapes(U))


def test_predicted_route_by_hand():
    """A few routes worked out by hand from the header, one per condition."""
    h = [[100, -7], [3, 4], [5, 6]]
    X = 1 << 20
    pr = ic.predicted_route
    # 3 taps at U = 2, c0 = 1: phase 0 is tap 1 on frame i, phase 1 taps 0 and 2 on frames i + 1 and i: W = 2
    assert pr(X, X, 1, 100, h, 2) == (ic.FAST, 2)
    # at U = 16: phases 0 and 1 are taps 1 and 2 on frame i, phase 15 tap 0 on frame i + 1, the rest empty
    assert pr(X, X + 4, 1, 100, h, 16) == (ic.FAST, 2)                # y at any int32 address
    assert pr(X, X, 1, 100, [[1, 2]], 16) == (ic.FAST, 1)
    assert pr(X, X, 0, 100, h, 2) == (ic.NONE, 0)
    assert pr(X, X, 3, 0, h, 2) == (ic.NONE, 0)
    assert pr(X, X, 1, 100, h, 1) == (ic.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 17) == (ic.GENERIC32, 0)
    assert pr(X + 4, X, 1, 100, h, 2) == (ic.GENERIC32, 0)
    assert pr(X + 2, X, 1, 100, h, 2) == (ic.GENERIC64, 0)
    assert pr(X, X, 3, 102, h, 2) == (ic.GENERIC32, 0)                # rows of 4k + 2 frames
    assert pr(X, X, 3, 104, h, 2) == (ic.FAST, 2)
    assert pr(X, X, 1, 100, h, 2, 12, 32, ic.OUT_U8_SAT) == (ic.GENERIC32, 0)
    assert pr(X, X, 1, 100, [[1, 2]] * 64, 2) == (ic.FAST, 33)        # 32 per phase, c0 = 32 even: W = 32
    assert pr(X, X, 1, 100, [[1, 2]] * 65, 2) == (ic.GENERIC32, 0)    # 33 per phase
    assert pr(X, X, 1, 100, [[1, 2]] * 128, 4) == (ic.FAST, 33)
    assert pr(X, X, 1, 100, [[1, 2]] * 129, 16) == (ic.GENERIC32, 0)  # 129 taps
    assert pr(X, X, 1, 100, [[1, 2]] * 128, 16) == (ic.FAST, 8)
    # 10 taps at U = 2, c0 = 5: phase 0 is taps 1, 3, .. on frames i + 2 .. i - 2, phase 1 taps 0, 2, .. on i + 3 .. i - 1
    assert pr(X, X, 1, 100, [[1, 2]] * 10, 2) == (ic.FAST, 6)
    assert pr(X, X, 1, 100, [[32767, -32767]], 2) == (ic.FAST, 1)
    assert pr(X, X, 1, 100, [[1, -32768]], 2) == (ic.GENERIC64, 0)
    assert pr(X, X, 1, 100, [[32768, 0]], 2) == (ic.GENERIC64, 0)
    assert pr(X, X, 1, 100, h, 2, 32, 32) == (ic.GENERIC64, 0)        # frac 32
    assert pr(X, X, 1, 100, h, 2, 12, 33) == (ic.GENERIC64, 0)
    assert pr(X, X, 1, 100, h, 2, 12, 64) == (ic.GENERIC64, 0)
    assert pr(X, X, 1, 1 << 40, h, 2) == (ic.GENERIC32, 0) and pr(X, X, 1, (1 << 40) - 1, h, 2)[0] == ic.FAST
    assert pr(X, X, 1 << 21, 1 << 21, h, 2) == (ic.GENERIC32, 0)      # 2^21 rows x 2^10 workgroups
    assert pr(X, X, (1 << 21) - 4, 1 << 21, h, 2)[0] == ic.FAST
    big = [[2**31 - 1, -(2**31 - 1)]] * (2**16 + 9)
    assert pr(X, X, 1, 100, big, 2, 12, 64) == (ic.GENERIC128, 0)
    assert pr(X, X, 1, 100, big, 2, 12, 63) == (ic.GENERIC64, 0)
    assert pr(X, X, 1, 100, big[:2**16 - 1], 2, 12, 64) == (ic.GENERIC64, 0)  # 2 (2^16 - 1)(2^31 - 1) 2^15 < 2^63
