"""CPU self-test of tests/cext_threshold_cases.py (the cases and references of
tests/test_gpu_cext_thresholds.py).  No GPU.

The needs_wide cases are held to what they claim -- the tap sums are 2^48 - 1 and 2^48 on exact
Python ints, the outputs whose window lies on -32768 samples sum to exactly 2^63 - 32768 and 2^63 in
the part the variant names, the routes the helpers predict are GENERIC64 and GENERIC128 -- and the
three references to each other: the staged exact sums equal the C oracle on the accept side (where
its 64-bit sums are exact), and ``oracle_kept`` equals the libraries' ``want`` where that is cheap.
The dot2_ok pairs: each first member on a v_dot2 route, each second on GENERIC64, by predicted_route
and by the library's own route query (which needs no device).
"""
from __future__ import annotations

import numpy as np
import pytest

import big_index_cases as bic
import cext_threshold_cases as tc

X, Y, HI, HO = 1 << 20, 1 << 21, 1 << 22, 1 << 23  # aligned addresses


@pytest.mark.parametrize("lib,variant,side", tc.wide_ids(), ids=["-".join(i) for i in tc.wide_ids()])
def test_wide_case_is_at_the_threshold(lib, variant, side):
    w = tc.wide_case(lib, variant, side)
    U, D, phase = tc.RATES[lib]
    # the taps: exact Python-int sums, one polyphase branch, the signs of the variant
    total = sum(abs(int(v)) for v in w.hq.reshape(-1))
    assert total == (1 << 48) - (side == "accept") and (total * 32768 >= 1 << 63) == (side == "reject")
    K = np.flatnonzero((w.hq != 0).any(axis=1))
    assert K.size == tc.N_WIDE >= (1 << 16) + 1 and np.abs(w.hq).max() == tc.PART_MAX
    assert set(K % U) == {tc.BRANCH if U > 1 else 0} and K[-1] == w.hq.shape[0] - 1
    assert (w.hq[:, 0] <= 0).all() and ((w.hq[:, 1] <= 0).all() if variant == "im" else (w.hq[:, 1] >= 0).all())
    assert bic.cdecim_cases.sum_can_pass_2_63(w.hq) == (side == "reject")  # the helpers' restated bound
    # the samples: -32768 but for a few near both row ends; the stream's history too, 2^16 frames and more
    row = np.concatenate([w.hist, w.x], axis=1) if w.hist is not None else w.x
    odd = np.flatnonzero(row[0] != -32768)
    assert 40 <= odd.size <= 80 and all(v < 2 * tc.ENDS or v >= row.size - 2 * tc.ENDS for v in odd)
    assert (w.hist is None) == (lib != "cstream") and (w.hist is None or w.hist.shape[1] // 2 == w.hq.shape[0] - 1 >= 1 << 16)
    # the outputs: about COMPARED of them, a good part with the whole window on -32768 samples, and
    # those sum to exactly the target in the variant's part
    assert 1000 <= w.outputs.size <= 1100 and len(w.sums) == w.outputs.size
    part = 0 if variant == "re" else 1
    assert w.target == ((1 << 63) - 32768 if side == "accept" else 1 << 63)
    assert int(w.pure.sum()) >= 256 and all(w.sums[j][part] == w.target for j in np.flatnonzero(w.pure))
    assert all(-(1 << 63) <= s <= w.target for pair in w.sums for s in pair)
    assert any(0 < s[part] < w.target for s in w.sums)  # ... and the others to a little less
    # the two sides of a pair differ in one tap part by one
    other = tc.wide_case(lib, variant, "reject" if side == "accept" else "accept")
    assert np.array_equal(other.x, w.x) and int(np.abs(other.hq - w.hq).sum()) == 1
    # the routes, by the helpers' predicted_route: the threshold alone decides, x at any address
    for frac, acc, stage in tc.WIDE_STAGES:
        for x_addr in (X, X + 4, X + 2):
            got = tc.predicted(lib, tc.addrs_of(lib, x_addr, Y, HI, HO), 1, w.width, w.hq, frac, acc, stage)
            assert got == (w.route, 0), (frac, acc, x_addr, got)
        assert tc.predicted(lib, tc.addrs_of(lib, X, Y, HI, HO), 1, w.width, w.hq, frac, 63, stage) == (tc.GENERIC64, 0)
    # what the reject side's target becomes: at acc 64 the reference wraps 2^63 to -2^63 itself
    if side == "reject":
        j = int(np.flatnonzero(w.pure)[0])
        got = [int(tc.staged([w.sums[j]], *s)[0, part]) for s in tc.WIDE_STAGES]
        assert got == [0, 255, 1 << 23, 1 << 23]


@pytest.mark.parametrize("lib,variant", [(lib, v) for lib in tc.LIBS for v in ("re", "im")])
def test_accept_side_sums_equal_the_c_oracle(lib, variant):
    """Below 2^63 the C oracle's 64-bit sums are exact: the staged Python-int sums must equal it."""
    w = tc.wide_case(lib, variant, "accept")
    runs = tc.oracle_runs(w.outputs.size)
    U = tc.RATES[lib][0]  # the middle run: whole windows on -32768 (where U > 1, the outputs of the taps' branch)
    assert int(w.pure[runs[1]].sum()) == 48 // U and not w.pure[runs[0]].all() and not w.pure[runs[2]].all()
    for frac, acc, stage in tc.WIDE_STAGES:
        at, ref = tc.oracle_spots(w, frac, acc, stage)
        assert at.size == 96 and np.array_equal(tc.staged(w.sums, frac, acc, stage)[at], ref), (frac, acc, stage)


@pytest.mark.parametrize("lib", tc.LIBS)
def test_the_model_and_oracle_kept_equal_want(lib):
    """At sizes where the libraries' whole-row ``want`` is cheap: every kept output of the model, as
    staged exact sums and as oracle_kept, equals it; taps with zeros, rows shorter than the taps."""
    rng = np.random.default_rng(7 + tc.LIBS.index(lib))
    U, D, phase = tc.RATES[lib]
    for L, width in ((1, 9), (5, 40), (8, 3), (33, 50), (12, 64)):
        hq = rng.integers(-(1 << 31) + 1, 1 << 31, (L, 2))
        hq[rng.integers(0, L, L // 3)] = 0
        hq[L - 1] = (-5, 7)
        x = rng.integers(-32768, 32768, (1, 2 * width), dtype=np.int16)
        hist = bic.cstream_cases.hostile_history(rng, 1, L - 1) if lib == "cstream" else None
        R = tc.model_row(lib, x, hist)
        for frac, acc, stage in ((12, 32, tc.I32), (40, 64, tc.I32), (20, 40, tc.U8), (12, 24, tc.I32)):
            want, _ = tc.reference(lib, x, hist, hq, frac, acc, stage)
            idx = tc.model_index(lib, L, np.arange(want.shape[1] // 2))
            assert idx.size
            sums, _ = tc.exact_sums(R, hq, idx)
            assert np.array_equal(tc.staged(sums, frac, acc, stage), want.reshape(-1, 2)), (L, width, frac, acc)
            assert np.array_equal(tc.oracle_kept(R, hq, idx, frac, acc, stage), want.reshape(-1, 2)), (L, width, frac, acc)
            some = idx[1::3] if idx.size > 3 else idx
            assert np.array_equal(tc.oracle_kept(R, hq, some, frac, acc, stage), want.reshape(-1, 2)[1::3] if idx.size > 3
                                  else want.reshape(-1, 2))


def test_exact_stage_by_hand():
    assert tc.exact_stage(1 << 63, 12, 64, tc.U8) == 0 and tc.exact_stage(1 << 63, 12, 65, tc.U8) == 255
    assert tc.exact_stage(1 << 63, 40, 65, tc.I32) == 1 << 23 == tc.exact_stage((1 << 63) - 32768, 40, 64, tc.I32)
    assert tc.exact_stage(-(1 << 63), 40, 64, tc.I32) == -(1 << 23) and tc.exact_stage(2047, 12, 32, tc.I32) == 0
    assert tc.exact_stage(2048, 12, 32, tc.I32) == 1 and tc.exact_stage(-2049, 12, 32, tc.I32) == -1
    assert tc.exact_stage((1 << 31) + 5, 1, 32, tc.I32) == -(1 << 30) + 3  # wrapped to 32 bits first


@pytest.mark.parametrize("lib", tc.LIBS)
def test_dot2_pairs_straddle_the_limits(lib):
    """Each pair differs in the one thing its name says; the first member is on FAST (rows of 4 k
    frames) or GENERIC32 (rows of 4 k + 2), the second on GENERIC64, by the helper's predicted_route
    and by the library's own route query."""
    ext = bic.CEXT[lib][0]
    pairs = tc.dot2_pairs(np.random.default_rng(5))
    assert [n for n, _, _ in pairs] == ["+32767 | +32768", "-32767 | -32768", "acc 32 | 33", "frac 31 | 32"]
    (a, b), (c, d) = (pairs[0][1:], pairs[1][1:])
    assert (a[0].max(), b[0].max(), c[0].min(), d[0].min()) == (32767, 32768, -32767, -32768)
    assert (a[1:], b[1:], c[1:], d[1:]) == ((12, 32),) * 4
    assert [(s[1:], f[1:]) for _, s, f in pairs[2:]] == [((12, 32), (12, 33)), ((31, 32), (32, 32))]
    for _, stay, fall in pairs:
        for h in (stay[0], fall[0]):
            assert h.shape == (tc.DOT2_TAPS, 2) and int((np.abs(h) == 32767).sum()) >= 2 * tc.DOT2_TAPS - 2
    for (rows, width), on in zip(tc.DOT2_SHAPES, (tc.FAST, tc.GENERIC32)):
        assert rows > 1 and (width % 4 == 0) == (on == tc.FAST)
        addrs = tc.addrs_of(lib, X, Y, HI, HO)
        for name, stay, fall in pairs:
            got = tc.predicted(lib, addrs, rows, width, stay[0], *stay[1:], tc.I32)
            assert got[0] == on and (got[1] > 0) == (on == tc.FAST), (name, got)
            assert tc.predicted(lib, addrs, rows, width, fall[0], *fall[1:], tc.I32) == (tc.GENERIC64, 0), name
            for hq, frac, acc in (stay, fall):
                asked = ext.route(*addrs, rows, width, hq, *tc.rate_args(lib), frac, acc, tc.I32)
                assert tuple(asked) == tc.predicted(lib, addrs, rows, width, hq, frac, acc, tc.I32), name
