"""The rational resampling complex-tap FIR's reference and predicted dispatch
(tests/cresample_cases.py), held against the contract written as plain Python ints before any GPU
test leans on them.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings

import cdecim_cases
import cinterp_cases
import cplx_ref
import cresample_cases as cc
from oracle import c_oracle

RATES = (1, 2, 3, 4, 16)


@pytest.mark.parametrize("D", RATES)
@pytest.mark.parametrize("U", RATES)
def test_want_is_the_polyphase_loop(U, D):
    """want (the C oracle on the stuffed signal, sliced) == want_loop (the header's polyphase formula,
    no stuffed signal): every phase, taps 1 .. 2 U + 3 (empty phases where taps < U, both parities of
    taps / 2), rows of 1, 2, taps - 1 and 9 frames, a row with mid_width <= phase among them."""
    rng = np.random.default_rng(100 * U + D)
    empty = 0
    for L in range(1, 2 * U + 4):
        hq = rng.integers(-32767, 32768, (L, 2))
        for width in sorted({1, 2, max(1, L - 1), 9}):
            x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
            x[0, :2] = (-32768, 32767)
            full = cinterp_cases.want(x, hq, U, 9, 32)
            for phase in range(D):
                loop = cc.want_loop(x, hq, U, D, phase, 9, 32)
                ow = cc.out_width(width, U, D, phase)
                assert loop.shape == (2, 2 * ow) and loop.dtype == np.int32
                assert ow == (-(-(width * U - phase) // D) if width * U > phase else 0)
                empty += ow == 0
                assert np.array_equal(cc.sliced(full, D, phase), loop), (U, D, phase, L, width)
            phase = int(rng.integers(0, D))
            assert np.array_equal(cc.want(x, hq, U, D, phase, 3, 24), cc.want_loop(x, hq, U, D, phase, 3, 24)), (U, D, L, width)
    assert (empty > 0) == (U < D)  # mid_width <= phase happens wherever it can: one frame, U <= phase < D


@pytest.mark.parametrize("stage", [cc.OUT_I32, cc.OUT_U8_SAT])
@pytest.mark.parametrize("acc", [24, 32, 40, 64])
def test_want_is_the_loop_at_every_stage_and_width_of_sum(acc, stage):
    rng = np.random.default_rng(100 * acc + stage)
    frac = 5 if stage == cc.OUT_U8_SAT else 9
    for U, D, phase, L, width in ((2, 3, 1, 5, 7), (3, 2, 0, 8, 33), (4, 6, 5, 2, 5), (7, 5, 2, 33, 6), (16, 15, 14, 17, 3), (1, 1, 0, 4, 9)):
        x = rng.integers(-32768, 32768, (2, 2 * width), dtype=np.int16)
        hq = rng.integers(-40, 41, (L, 2)) if stage == cc.OUT_U8_SAT else rng.integers(-32767, 32768, (L, 2))
        got = cc.want(x, hq, U, D, phase, frac, acc, stage)
        assert got.dtype == (np.uint8 if stage == cc.OUT_U8_SAT else np.int32)
        assert np.array_equal(got, cc.want_loop(x, hq, U, D, phase, frac, acc, stage)), (U, D, L, width)


def test_want_loop_past_2_63():
    """Taps of +-(2^31 - 1): want_loop against the sliced interpolator loop, both unbounded ints."""
    rng = np.random.default_rng(7)
    hq = np.where(rng.integers(0, 2, (9, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    x = np.full((1, 2 * 6), 32767, np.int16)
    for U, D, phase in ((1, 1, 0), (2, 3, 1), (3, 2, 1)):
        up = cinterp_cases.want_loop(x, hq, U, 40, 80)
        assert np.array_equal(cc.want_loop(x, hq, U, D, phase, 40, 80), cc.sliced(up, D, phase))


def test_the_four_identities():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, (6, 2 * 23), dtype=np.int16)
    hq = rng.integers(-3000, 3001, (7, 2))
    for frac, acc, stage in ((12, 32, cc.OUT_I32), (6, 24, cc.OUT_U8_SAT), (20, 40, cc.OUT_I32)):
        bits = (frac, acc, stage)
        for U in (1, 2, 5, 16):  # decim = 1 is the interpolator
            assert np.array_equal(cc.want(x, hq, U, 1, 0, *bits), cinterp_cases.want(x, hq, U, *bits))
            assert np.array_equal(cc.want_loop(x, hq, U, 1, 0, *bits), cinterp_cases.want(x, hq, U, *bits))
        for D in (1, 2, 5, 16):  # up = 1 is the decimator
            for phase in {0, D // 2, D - 1}:
                ref = cdecim_cases.want(x, hq, D, phase, *bits)
                assert np.array_equal(cc.want(x, hq, 1, D, phase, *bits), ref)
                assert np.array_equal(cc.want_loop(x, hq, 1, D, phase, *bits), ref)
        # up = decim = 1 is the full-rate filter
        assert np.array_equal(cc.want_loop(x, hq, 1, 1, 0, *bits), cplx_ref.want(x, hq, *bits))
        # hi = 0 is the real oracle with two channels on the stuffed signal, sliced
        hr = hq.copy()
        hr[:, 1] = 0
        for U, D, phase in ((2, 3, 1), (3, 2, 0), (16, 5, 4)):
            real = c_oracle().fir1d_rows(cinterp_cases.stuffed(x, U), hr[:, 0], frac, acc, stage, channels=2)
            assert np.array_equal(cc.want_loop(x, hr, U, D, phase, *bits), cc.sliced(real, D, phase)), (U, D, phase)


def test_out_width_buckets_and_shape_lists():
    for U in range(1, 18):
        for D in range(1, 18):
            for phase in range(D):
                for width in range(0, 12):
                    mid = width * U
                    assert cc.out_width(width, U, D, phase) == ((mid - phase + D - 1) // D if mid > phase else 0)
    assert [cc.periods(D) for D in (2, 3, 4, 5, 16)] == [512, 512, 256, 256, 256]
    assert [cc.tile(U, 2) for U in (2, 3, 4, 5, 16)] == [512, 512, 512, 256, 256] and cc.tile(2, 4) == 256
    for U in range(2, 17):
        for D in range(2, 17):
            P, T = cc.periods(D), cc.tile(U, D)
            assert P * D * 4 >= 4096 and P % T == 0 and (T * U * 8 <= 16384 or T == 256)
            for phase in (0, D - 1):
                for L in range(1, cc.fast_max_taps(U) + 1):
                    ph = cc.phases(L, U, D, phase)
                    need = max(n for _, _, n in ph)
                    assert need <= -(-L // U) <= 32 and cc.bucket(L, U, D, phase) >= max(need, 1)
                    # every tap is met by at most one phase slot, and a window start is at most D + 1 past the lowest
                    starts = [c - n + 1 for _, c, n in ph if n]
                    assert not starts or max(starts) - min(starts) <= D + 1
            edges = cc.edge_widths(U, D)
            for e in cc.edge_out_widths(U, D):
                w = -(-e * D // U)
                assert {w, w + 1} <= set(edges) and (w == 1 or w - 1 in edges)
                assert cc.out_width(w, U, D, 0) >= e >= cc.out_width(w - 1, U, D, 0)  # the edge lies in the row from w on
            assert all(w % cc.ROW_UNIT == 0 for _, w in cc.multi_row_shapes(U, D))
    # all phases empty: one tap at U = 4, D = 2, phase 1 meets only stuffed zeros
    assert cc.bucket(1, 4, 2, 1) == 1 and all(n == 0 for _, _, n in cc.phases(1, 4, 2, 1))
    assert cc.bucket(64, 2, 3, 0) == 32 and cc.bucket(128, 16, 15, 0) == 8 and cc.bucket(72, 3, 2, 0) == 24


def test_predicted_route_by_hand():
    """A few routes worked out by hand from the header, one per condition."""
    h = [[100, -7], [3, 4], [5, 6]]
    X = 1 << 20
    pr = cc.predicted_route
    # 3 taps at U = 3, D = 2, c0 = 1: a_q = 1, 3, 5 -> p_q = 1, 0, 2: one tap per phase
    assert pr(X, X, 1, 100, h, 3, 2) == (cc.FAST, 1)
    # at U = 2, D = 3: a_q = 1, 4 -> p_q = 1, 0: phase 0 is tap 1, phase 1 taps 0 and 2
    assert pr(X, X + 4, 1, 100, h, 2, 3) == (cc.FAST, 2)                # y at any int32 address
    assert pr(X, X, 0, 100, h, 3, 2) == (cc.NONE, 0)
    assert pr(X, X, 3, 0, h, 3, 2) == (cc.NONE, 0)
    assert pr(X, X, 3, 1, h, 2, 5, 2) == (cc.NONE, 0)                  # mid_width = 2 <= phase
    assert pr(X, X, 3, 1, h, 2, 5, 1)[0] != cc.NONE
    assert pr(X, X, 1, 100, h, 1, 2) == (cc.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 2, 1) == (cc.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 17, 2) == (cc.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 2, 17) == (cc.GENERIC32, 0)
    assert pr(X, X, 1, 100, h, 16, 16, 15)[0] == cc.FAST
    assert pr(X + 4, X, 1, 100, h, 3, 2) == (cc.GENERIC32, 0)
    assert pr(X + 2, X, 1, 100, h, 3, 2) == (cc.GENERIC64, 0)
    assert pr(X, X, 3, 102, h, 3, 2) == (cc.GENERIC32, 0)                # rows of 4k + 2 frames
    assert pr(X, X, 3, 104, h, 3, 2) == (cc.FAST, 1)
    assert pr(X, X, 1, 100, h, 3, 2, 0, 12, 32, cc.OUT_U8_SAT) == (cc.GENERIC32, 0)
    assert pr(X, X, 1, 100, [[1, 2]] * 64, 2, 3) == (cc.FAST, 32)        # 32 per phase
    assert pr(X, X, 1, 100, [[1, 2]] * 65, 2, 3) == (cc.GENERIC32, 0)    # 33 per phase
    assert pr(X, X, 1, 100, [[1, 2]] * 128, 4, 3) == (cc.FAST, 32)
    assert pr(X, X, 1, 100, [[1, 2]] * 129, 16, 3) == (cc.GENERIC32, 0)  # 129 taps
    assert pr(X, X, 1, 100, [[1, 2]] * 128, 16, 3) == (cc.FAST, 8)
    assert pr(X, X, 1, 100, [[32767, -32767]], 3, 2) == (cc.FAST, 1)
    assert pr(X, X, 1, 100, [[1, -32768]], 3, 2) == (cc.GENERIC64, 0)
    assert pr(X, X, 1, 100, [[32768, 0]], 3, 2) == (cc.GENERIC64, 0)
    assert pr(X, X, 1, 100, h, 3, 2, 0, 32, 32) == (cc.GENERIC64, 0)     # frac 32
    assert pr(X, X, 1, 100, h, 3, 2, 0, 12, 33) == (cc.GENERIC64, 0)
    assert pr(X, X, 1, 1 << 40, h, 3, 2) == (cc.GENERIC32, 0) and pr(X, X, 1, (1 << 40) - 1, h, 3, 2)[0] == cc.FAST
    # U = 2, D = 2: 1024 output frames per workgroup, a row of 2^21 frames is 2^11 workgroups
    assert pr(X, X, 1 << 20, 1 << 21, h, 2, 2) == (cc.GENERIC32, 0)      # 2^20 rows x 2^11 workgroups
    assert pr(X, X, (1 << 20) - 1, 1 << 21, h, 2, 2)[0] == cc.FAST
    big = [[2**31 - 1, -(2**31 - 1)]] * (2**16 + 9)
    assert pr(X, X, 1, 100, big, 3, 2, 0, 12, 64) == (cc.GENERIC128, 0)
    assert pr(X, X, 1, 100, big, 3, 2, 0, 12, 63) == (cc.GENERIC64, 0)
    assert pr(X, X, 1, 100, big[:2**16 - 1], 3, 2, 0, 12, 64) == (cc.GENERIC64, 0)


def test_property_cases_cover_every_reason_and_stay_small():
    """A seeded draw of 400 cases: every `why` occurs, between a third and two thirds predict FAST, the
    route is FAST exactly when nothing keeps the case off it, and the size cap holds."""
    seen = []

    @seed(20260101)
    @settings(max_examples=400, database=None, deadline=None, derandomize=False,
              suppress_health_check=list(HealthCheck))
    @given(cc.property_case())
    def draw(case):
        why, c = case
        route, _ = cc.predicted_route(c.x_lead, c.y_lead, c.rows, c.width, np.asarray(c.hq, dtype=np.int64), c.up, c.decim,
                                      c.phase, c.frac, c.acc, c.stage)
        assert route != cc.NONE and (route == cc.FAST) == (why == ""), (why, c, route)
        assert c.rows * c.width * c.up <= cc.PROPERTY_MAX_PRODUCT and 0 <= c.phase < c.decim
        seen.append((why, route))

    draw()
    assert len(seen) >= 400
    assert {w for w, _ in seen} == set(cc.WHY), sorted({w for w, _ in seen})
    fast = sum(r == cc.FAST for _, r in seen) / len(seen)
    assert 1 / 3 <= fast <= 2 / 3, fast
