"""The decimating complex-tap FIR's reference and predicted dispatch (tests/cdecim_cases.py), held
against the contract written as plain Python ints before any GPU test leans on them.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import cdecim_cases as dc
from cplx_ref import cplx_loop

WIDTHS = (1, 2, 7, 33)
TAPS = (1, 2, 5, 8)
DECIMS = (1, 2, 3, 5, 16)


@pytest.mark.parametrize("stage", [dc.OUT_I32, dc.OUT_U8_SAT])
@pytest.mark.parametrize("acc", [24, 32, 40])
def test_want_is_the_sliced_loop(acc, stage):
    """want == cplx_loop viewed as frames [..., phase::D, :]: rows of 1, 2, 7 and 33 frames, 1, 2, 5
    and 8 taps, D in 1, 2, 3, 5, 16 with every phase."""
    rng = np.random.default_rng(100 * acc + stage)
    frac = 5 if stage == dc.OUT_U8_SAT else 9  # small enough that the u8 stage sees values inside (0, 255) too
    for width in WIDTHS:
        x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
        x[0, :2] = (-32768, 32767)
        for L in TAPS:
            hq = rng.integers(-40, 41, (L, 2)) if stage == dc.OUT_U8_SAT else rng.integers(-32767, 32768, (L, 2))
            full = cplx_loop(x, hq, frac, acc, stage).reshape(2, width, 2)
            for D in DECIMS:
                for phase in range(D):
                    got = dc.want(x, hq, D, phase, frac, acc, stage)
                    ref = np.ascontiguousarray(full[:, phase::D, :]).reshape(2, -1)
                    assert got.dtype == ref.dtype and got.shape == ref.shape == (2, 2 * dc.out_width(width, D, phase))
                    assert np.array_equal(got, ref), (width, L, D, phase)
                    assert np.array_equal(dc.want_loop(x, hq, D, phase, frac, acc, stage), ref)


def test_out_width_and_widths_for():
    for D in range(1, 18):
        for phase in range(D):
            for width in range(0, 41):
                want = (width - phase + D - 1) // D if width > phase else 0  # the header's formula
                assert dc.out_width(width, D, phase) == want
            for ow in (1, 2, 63, 512, 513):
                for slack in {0, D - 1}:
                    assert dc.out_width(dc.width_for(ow, D, phase, slack), D, phase) == ow


def test_edge_lists_hold_the_kernels_edges():
    for D in (2, 3, 4, 8, 16):
        G = dc.tiles_per_group(D)
        assert G == max(1, 16 // D) and G * D <= 16
        edges = dc.edge_out_widths(D)
        for mark in (1, dc.W, 257, dc.T, G * dc.T, 2 * G * dc.T):
            assert {mark, mark + 1} <= set(edges) and (mark == 1 or mark - 1 in edges)
        # the widest row is about 16 Ki frames at every D
        assert 15000 < dc.width_for(max(edges), D, D - 1) <= 2 * 16 * dc.T + 2 * D
        assert all(w % dc.ROW_UNIT == 0 for _, w in dc.multi_row_shapes(D))


def test_predicted_route_by_hand():
    """A few routes worked out by hand from the header, one per condition."""
    h = [[100, -7], [3, 4], [5, 6]]
    X = 1 << 20
    pr = dc.predicted_route
    assert pr(X, X, 1, 100, h, 2) == (dc.FAST, 4)
    assert pr(X, X + 4, 1, 100, h, 16, 15) == (dc.FAST, 4)            # y at any int32 address
    assert pr(X, X, 1, 100, h, 2, 0, 12, 32, dc.OUT_I32) == (dc.FAST, 4)
    assert pr(X, X, 1, 15, h, 16, 15) == (dc.NONE, 0)                 # phase >= width
    assert pr(X, X, 0, 100, h, 2) == (dc.NONE, 0)
    assert pr(X, X, 1, 100, h, 1) == (dc.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 17) == (dc.GENERIC32, 0)
    assert pr(X + 4, X, 1, 100, h, 2) == (dc.GENERIC32, 0)
    assert pr(X + 2, X, 1, 100, h, 2) == (dc.GENERIC64, 0)
    assert pr(X, X, 3, 102, h, 2) == (dc.GENERIC32, 0)                # rows of 4k + 2 frames
    assert pr(X, X, 3, 104, h, 2) == (dc.FAST, 4)
    assert pr(X, X, 1, 100, h, 2, 0, 12, 32, dc.OUT_U8_SAT) == (dc.GENERIC32, 0)
    assert pr(X, X, 1, 100, [[1, 2]] * 64, 2) == (dc.FAST, 64)
    assert pr(X, X, 1, 100, [[1, 2]] * 65, 2) == (dc.GENERIC32, 0)
    assert pr(X, X, 1, 100, [[32767, -32767]], 2) == (dc.FAST, 2)
    assert pr(X, X, 1, 100, [[1, -32768]], 2) == (dc.GENERIC64, 0)
    assert pr(X, X, 1, 100, [[32768, 0]], 2) == (dc.GENERIC64, 0)
    assert pr(X, X, 1, 100, h, 2, 0, 32, 32) == (dc.GENERIC64, 0)     # frac 32
    assert pr(X, X, 1, 100, h, 2, 0, 12, 33) == (dc.GENERIC64, 0)
    assert pr(X, X, 1, 100, h, 2, 0, 12, 64) == (dc.GENERIC64, 0)
    big = [[2**31 - 1, -(2**31 - 1)]] * (2**16 + 9)
    assert pr(X, X, 1, 100, big, 2, 0, 12, 64) == (dc.GENERIC128, 0)
    assert pr(X, X, 1, 100, big, 2, 0, 12, 63) == (dc.GENERIC64, 0)
    assert pr(X, X, 1, 100, big[:2**16 - 1], 2, 0, 12, 64) == (dc.GENERIC64, 0)  # 2 (2^16 - 1)(2^31 - 1) 2^15 < 2^63
