"""The streaming resampler's test helper (tests/crstream_cases.py) held to itself, without a GPU or the
library: identity 2 of include/fir_crstream.h (want_block, over the C oracle) against the causal
formula in Python ints (want_block_loop), split invariance of the reference, next_phase in [0, D),
identity 3 (up = 1 is the streaming decimator's reference), and the bounds the fast kernel's causal
plan rests on (S >= -H, k0 <= D) for every rate, tap count and phase of the fast route."""
from __future__ import annotations

import numpy as np
import pytest

import crstream_cases as rs
import cstream_cases as sc

# (U, D, L): H * U < L // 2 (L = 3, U = 4 and L = 5, U = 3), L <= U (H = 0), L = 1, U or D of 1, L a multiple of U
SMALL = [(4, 3, 3), (3, 2, 5), (4, 3, 4), (5, 2, 2), (3, 2, 1), (1, 3, 7), (3, 1, 7), (1, 1, 4), (2, 3, 9), (3, 2, 12),
         (16, 15, 33), (2, 16, 6), (16, 2, 40), (17, 5, 20), (3, 17, 8)]


def _same(a, b, what):
    assert a[0].dtype == b[0].dtype and a[0].shape == b[0].shape, what
    assert np.array_equal(a[0], b[0]), (what, "y")
    assert np.array_equal(a[1], b[1]), (what, "hist_out")
    assert a[2] == b[2], (what, "next_phase")


@pytest.mark.parametrize("U,D,L", SMALL)
def test_identity_2_is_the_causal_formula(U, D, L):
    rng = np.random.default_rng(1000 * U + 10 * D + L)
    H = rs.hist_frames(L, U)
    assert (U, D, L) != (4, 3, 3) or (H == 0 and H * U < L // 2)
    hq = rs.taps(rng, L)
    for rows, width in ((1, 1), (2, 2), (1, H), (2, H + 1), (3, 19)):
        x = rs.frames(rng, rows, width)
        for phase in sorted({0, D - 1, D // 2}):
            for hist in (None, rs.hostile_history(rng, rows, H)):
                for frac, acc, stage in ((12, 32, rs.OUT_I32), (3, 20, rs.OUT_I32), (16, 40, rs.OUT_U8_SAT)):
                    a = rs.want_block(x, hist, hq, U, D, phase, frac, acc, stage)
                    b = rs.want_block_loop(x, hist, hq, U, D, phase, frac, acc, stage)
                    _same(a, b, (U, D, L, rows, width, phase, hist is None, acc))
                    assert a[0].shape == (rows, 2 * rs.out_width(width, U, D, phase)) and a[1].shape == (rows, 2 * H)
                    assert 0 <= a[2] < D


def test_leading_axes_and_wide_sums():
    rng = np.random.default_rng(7)
    x, hq = rs.frames(rng, 6, 9).reshape(2, 3, 18), rs.taps(rng, 7)
    hist = rs.hostile_history(rng, 6, 2).reshape(2, 3, 4)
    a = rs.want_block(x, hist, hq, 3, 2, 1)
    b = rs.want_block_loop(x, hist, hq, 3, 2, 1)
    _same(a, b, "leading axes")
    assert a[0].shape == (2, 3, 2 * rs.out_width(9, 3, 2, 1)) and a[1].shape == (2, 3, 4)
    # a sum past 2^63 keeps its low bits in the loop (no int64 anywhere in it)
    big = np.full((5, 2), 2**31 - 1, dtype=object)
    y, _, _ = rs.want_block_loop(np.full((1, 8), 32767, np.int16), None, big, 1, 1, 0, 1, 100)
    assert y.dtype == np.int32


@pytest.mark.parametrize("U,D,L", SMALL)
def test_the_reference_is_split_invariant(U, D, L):
    rng = np.random.default_rng(2000 * U + 10 * D + L)
    H = rs.hist_frames(L, U)
    hq = rs.taps(rng, L)
    N = 41
    x = rs.frames(rng, 2, N)
    for hist in (None, rs.hostile_history(rng, 2, H)):
        for phase in (0, D - 1):
            one = rs.want_block(x, hist, hq, U, D, phase)
            for widths in ([1] * N, [N], [0, N, 0], rs.random_split(rng, N, 3 * D), rs.random_split(rng, N, H + 2)):
                for block in (rs.want_block, rs.want_block_loop):
                    got = rs.run_split(block, x, hist, hq, U, D, phase, widths)
                    _same(got, one, (U, D, L, phase, widths, block.__name__))


def test_next_phase_stays_in_range_and_counts_add_up():
    for U in range(1, 19):
        for D in range(1, 19):
            for phase in range(D):
                total = 0
                p = phase
                for width in (0, 1, 2, 5, 0, 17, 3):
                    ow = rs.out_width(width, U, D, p)
                    assert ow == len(range(p, width * U, D))
                    p = rs.next_phase(width, U, D, p)
                    assert 0 <= p < D
                    total += ow
                assert total == rs.out_width(28, U, D, phase) and p == rs.next_phase(28, U, D, phase)


@pytest.mark.parametrize("D,L", [(1, 5), (3, 1), (3, 8), (16, 33)])
def test_identity_3_up_1_is_the_streaming_decimator(D, L):
    rng = np.random.default_rng(30 + D + L)
    assert rs.hist_frames(L, 1) == L - 1
    hq = rs.taps(rng, L)
    x = rs.frames(rng, 2, 50)
    for hist in (None, rs.hostile_history(rng, 2, L - 1)):
        for phase in (0, D - 1):
            _same(rs.want_block(x, hist, hq, 1, D, phase), sc.want_block(x, hist, hq, D, phase), (D, L, phase))
            assert rs.next_phase(50, 1, D, phase) == sc.next_phase(50, D, phase)


def test_the_causal_plan_stays_inside_the_history_and_the_offset_table():
    """For every (L, U, D, phase) of the fast route: the lowest window starts at S >= -H, a window's
    first dword k0 = c - n + 1 - S is at most D, so k0 + bucket <= 16 + 32 window dwords; the frames a
    window's real taps meet are exactly the formula's (i - t with i = v D + c_q), and the bucket is the
    smallest that holds ceil((L - p) / U) of every phase that has a tap."""
    worst = 0
    for U in range(2, 17):
        for D in range(2, 17):
            for L in range(1, min(128, 32 * U) + 1):
                H = rs.hist_frames(L, U)
                for phase in range(D):
                    ph = rs.phases(L, U, D, phase)
                    S = rs.window_start(L, U, D, phase)
                    b = rs.bucket(L, U, D, phase)
                    assert -H <= S <= D - 1
                    for q, (p, c, n) in enumerate(ph):
                        j = phase + q * D
                        assert (p, c) == (j % U, j // U) and n == len(range(p, L, U))
                        if n:
                            k0 = c - n + 1 - S
                            assert 0 <= k0 <= D and n <= b
                            worst = max(worst, k0 + b)
                    assert b in rs.BUCKETS and (b == 1 or max(n for _, _, n in ph) > rs.BUCKETS[rs.BUCKETS.index(b) - 1])
    assert worst <= 16 + 32


def test_predicted_route_names_each_condition():
    X = 1 << 30
    rng = np.random.default_rng(3)
    hq = rs.taps(rng, 24)
    assert rs.predicted_route(X, X, X, X, 1, 4096, hq, 3, 2, 1) == (rs.FAST, 8)
    assert rs.predicted_route(X, X, X, X, 1, 0, hq, 3, 2, 1) == (rs.NONE, 0)
    assert rs.predicted_route(X, X + 2, X, X, 1, 4096, hq, 3, 2, 1) == (rs.GENERIC64, 0)
    assert rs.predicted_route(X, X + 2, X, X + 2, 1, 4096, hq[:3], 3, 2, 1) == (rs.FAST, 1)  # H = 0
    assert rs.predicted_route(X, X, X, X, 1, 4096, hq, 1, 2, 1) == (rs.GENERIC32, 0)
    assert rs.predicted_route(X, X, X, X, 1, 4096, hq, 3, 17, 1) == (rs.GENERIC32, 0)
    assert rs.predicted_route(X, X, X, X, 1, 4096, hq, 3, 2, 1, 12, 64) == (rs.GENERIC64, 0)
