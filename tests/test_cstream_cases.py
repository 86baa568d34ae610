"""tests/cstream_cases.py's references, without a GPU: ``want_block`` (identity 2 of
include/fir_cstream.h over the committed C oracle) against ``want_block_loop`` (the same over plain
Python ints) and against the header's defining causal sum written out directly, the split invariance
(identity 1) of the reference itself, and the range of next_phase."""
from __future__ import annotations

import numpy as np
import pytest

import cstream_cases as sc

I32, U8 = sc.OUT_I32, sc.OUT_U8_SAT


def _same3(a, b, what):
    assert a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]), (what, "y")
    assert a[1].dtype == b[1].dtype == np.int16 and np.array_equal(a[1], b[1]), (what, "hist_out")
    assert a[2] == b[2], (what, "next_phase")


def _causal(x, hist, hq, D, phase, frac, acc):
    """The header's sums as Python ints, int32 stage: wrap to acc bits, round half up by frac."""
    rows, width = x.shape[0], x.shape[1] // 2
    L = len(hq)
    H = L - 1
    X = np.concatenate([hist if hist is not None else np.zeros((rows, 2 * H), np.int16), x], axis=1).astype(object)
    out = []
    for r in range(rows):
        row = []
        for n in range(phase, width, D):
            re = sum(int(hq[k][0]) * X[r, 2 * (n - k + H)] - int(hq[k][1]) * X[r, 2 * (n - k + H) + 1] for k in range(L))
            im = sum(int(hq[k][0]) * X[r, 2 * (n - k + H) + 1] + int(hq[k][1]) * X[r, 2 * (n - k + H)] for k in range(L))
            for v in (re, im):
                if acc < 64:
                    v = (v + (1 << (acc - 1))) % (1 << acc) - (1 << (acc - 1))
                v = (v + (1 << (frac - 1))) >> frac
                row.append((v + (1 << 31)) % (1 << 32) - (1 << 31))
        out.append(row)
    return np.array(out, dtype=np.int64).astype(np.int32).reshape(rows, -1)


@pytest.mark.parametrize("L", range(1, 9))
def test_want_block_is_the_causal_sum_and_the_loop(L):
    rng = np.random.default_rng(100 + L)
    hq = sc.taps(rng, L)
    for D in range(1, 6):
        for phase in range(D):
            for width in (0, 1, 2, L - 1, L, 7, 23):
                x = sc.frames(rng, 2, width)
                for hist in (None, sc.hostile_history(rng, 2, L - 1)):
                    got = sc.want_block(x, hist, hq, D, phase)
                    _same3(got, sc.want_block_loop(x, hist, hq, D, phase), (L, D, phase, width))
                    assert np.array_equal(got[0], _causal(x, hist, hq.tolist(), D, phase, 12, 32)), (L, D, phase, width)
                    z = np.concatenate([hist if hist is not None else np.zeros((2, 2 * (L - 1)), np.int16), x], axis=1)
                    assert np.array_equal(got[1], z[:, z.shape[1] - 2 * (L - 1):])
    x, hist = sc.frames(rng, 2, 19), sc.hostile_history(rng, 2, L - 1)
    for frac, acc, stage in ((1, 17, I32), (31, 32, I32), (20, 40, I32), (12, 64, I32), (6, 32, U8)):
        h = sc.taps(rng, L, -40, 41) if stage == U8 else hq
        _same3(sc.want_block(x, hist, h, 3, 1, frac, acc, stage), sc.want_block_loop(x, hist, h, 3, 1, frac, acc, stage),
               (L, frac, acc, stage))
        _same3(sc.want_block_kept(x, hist, h, 3, 1, frac, acc, stage), sc.want_block_loop(x, hist, h, 3, 1, frac, acc, stage),
               (L, frac, acc, stage, "kept"))
    # int32-sized taps and no wrap: only the Python-int references are exact here
    big = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1)
    for hist in (None, sc.hostile_history(rng, 2, L - 1)):
        _same3(sc.want_block_kept(x, hist, big, 2, 1, 30, 64), sc.want_block_loop(x, hist, big, 2, 1, 30, 64), (L, "big"))


@pytest.mark.parametrize("L", range(1, 9))
def test_the_reference_is_split_invariant(L):
    rng = np.random.default_rng(200 + L)
    hq = sc.taps(rng, L)
    N = 61
    x = sc.frames(rng, 3, N)
    for D in range(1, 6):
        for phase in range(D):
            for hist in (None, sc.hostile_history(rng, 3, L - 1)):
                one = sc.want_block(x, hist, hq, D, phase)
                for hi in (1, 3, 2 * L, N):
                    widths = sc.random_split(rng, N, hi)
                    y, h_end, p_end = sc.run_split(sc.want_block, x, hist, hq, D, phase, widths)
                    _same3((y, h_end, p_end), one, (L, D, phase, widths))
                # zero-width blocks in front, in the middle and at the end
                y, h_end, p_end = sc.run_split(sc.want_block, x, hist, hq, D, phase, [0, 5, 0, 0, N - 5, 0])
                _same3((y, h_end, p_end), one, (L, D, phase, "zero widths"))


def test_next_phase_stays_in_range_and_continues_the_grid():
    for D in range(1, 18):
        for phase in range(D):
            for width in range(0, 50):
                p = sc.next_phase(width, D, phase)
                assert 0 <= p < D
                # the kept frames of two blocks are the kept frames of their concatenation
                for w2 in (0, 1, D, 13):
                    kept = list(range(phase, width, D)) + [width + n for n in range(p, w2, D)]
                    assert kept == list(range(phase, width + w2, D))
                    assert sc.next_phase(w2, D, p) == sc.next_phase(width + w2, D, phase)
