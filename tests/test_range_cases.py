"""CPU: the threshold table of tests/range_cases.py is what it claims to be, with NumPy and
oracle.fir_oracle only.  For every case:

* the restated predicate accepts the first configuration and rejects the second (and the
  conservative extension), and the two differ by one unit in one tap (of one factor for a
  rank-1 kernel, where a unit moves a whole column or row of taps);
* the exact sums over the worst-case rows / frames attain exactly the extremes the predicate
  computed, on both sides;
* the narrow form's model equals the oracle on the accepted side (and, where the proof is
  conservative, on the rejected side too) and differs from it somewhere on the rejected side
  (tight proofs) or on the conservative extension: no case is vacuous.
"""
from __future__ import annotations

import numpy as np
import pytest

import range_cases as rc
from oracle import fir_oracle as fo

CASES = {c.id: c for c in rc.CASES}


def _shape(case, side):
    if case.kind == "frame":
        return (29, 64)
    return max(256, 3 * case.filter_taps(side).size)


def _one_unit(a, b, unit) -> bool:
    d = np.asarray(b, np.int64) - np.asarray(a, np.int64)
    return np.count_nonzero(d) == 1 and int(np.abs(d).max()) == unit


@pytest.mark.parametrize("cid", list(CASES))
def test_pair_flips_by_one_unit(cid):
    c = CASES[cid]
    assert c.predicate(c.accept), "the accepted side is not accepted"
    assert not c.predicate(c.reject), "the rejected side is not rejected"
    assert (c.accept.frac, c.accept.acc) == (c.reject.frac, c.reject.acc)
    a, b = c.accept.taps, c.reject.taps
    fa = rc.rank1_factor(a) if c.kind == "frame" else None
    fb = rc.rank1_factor(b) if c.kind == "frame" else None
    if fa is not None and fb is not None:  # a rank-1 kernel: one unit in one tap of one factor
        row_step = np.array_equal(fa[0], fb[0]) and _one_unit(fa[1], fb[1], 1)
        col_step = np.array_equal(fa[1], fb[1]) and _one_unit(fa[0], fb[0], 1)
        assert row_step or col_step, (fa, fb)
    else:
        assert fa is None and fb is None
        assert _one_unit(a, b, c.unit), (a, b)
    if c.extra is not None:
        assert not c.predicate(c.extra) and rc.habs(c.extra.taps) > rc.habs(b)


@pytest.mark.parametrize("cid", list(CASES))
def test_worst_inputs_attain_the_extremes(cid):
    c = CASES[cid]
    for name, side in c.sides():
        x, _ = c.inputs(side, _shape(c, side))
        q = c.quantity(c.sums(x, side), side)
        vmax, vmin = c.bounds(side)
        assert (int(q.max()), int(q.min())) == (int(vmax), int(vmin)), (cid, name)


@pytest.mark.parametrize("cid", list(CASES))
def test_narrow_model_discriminates(cid):
    c = CASES[cid]
    differs = {}
    for name, side in c.sides():
        x, _ = c.inputs(side, _shape(c, side))
        differs[name] = any(not np.array_equal(c.narrow(x, side, st), c.oracle(x, side, st)) for st in c.stages)
    assert not differs["accept"], "the narrow form's model is wrong on the accepted side"
    if c.tight:
        assert differs["reject"], "tight proof: the narrow form must fail one unit past it"
    else:
        assert not differs["reject"], "marked conservative, but the narrow form already fails on the rejected side"
        assert differs["conservative"], "the conservative extension does not break the narrow form"
        # ... and it is the first that does: one unit less on the tap that grew is still right
        d = np.asarray(c.extra.taps, np.int64) - np.asarray(c.reject.taps, np.int64)
        if np.count_nonzero(d) == 1:  # (a rank-1 kernel grows by a column of taps: its steps are coarser)
            prev = rc.Side(c.extra.taps - np.sign(d), c.extra.frac, c.extra.acc)
            x, _ = c.inputs(prev, _shape(c, prev))
            assert all(np.array_equal(c.narrow(x, prev, st), c.oracle(x, prev, st)) for st in c.stages), \
                "the narrow form breaks before the extension"


@pytest.mark.parametrize("seam", rc.SEAMS, ids=[s["id"] for s in rc.SEAMS])
def test_seams_are_what_they_say(seam):
    assert [seam["value"](s) for s in seam["sides"]] == seam["expect"]


def test_every_source_row_has_cases():
    rows = {c.row for c in rc.CASES}
    assert rows == set(rc.ROWS)
    assert {s["row"] for s in rc.SEAMS} <= rows


def test_worst_rows_hit_every_phase():
    """The extreme lands on every residue n mod L below 16 (every lane and vector slot, even L too)."""
    for h in (np.array([3, -2, 5, 1]), np.array([-7, 2, 0, 4, -1, 9, 2])):
        x, names = rc.worst_rows_u8(h, 64)
        S = fo._mac_rows(x.astype(np.int64), h)
        L = h.size
        for p in range(L):
            n = np.arange(L + p, 64 - L, L)
            assert (S[names.index(f"high+{p}"), n] == 255 * rc.psum(h)).all()
            assert (S[names.index(f"low+{p}"), n] == 255 * rc.nsum(h)).all()
        xi, ni = rc.worst_rows_i16(h, 64)
        Si = fo._mac_rows(xi.astype(np.int64), h)
        assert Si.max() == 32767 * rc.psum(h) - 32768 * rc.nsum(h)
        assert Si.min() == -32768 * rc.psum(h) + 32767 * rc.nsum(h)
        assert {"zeros", "min", "max", "random", "random_ends", "high_near", "low_near"} <= set(ni)
    h2 = np.array([[1, -2, 3], [0, 5, -6], [7, 8, -9]])
    x2, n2 = rc.worst_frames_u8(h2, 12, 16)
    S2 = np.stack([rc.mac2d(f, h2) for f in x2])
    for p in range(9):
        dy, dx = p // 3, p % 3
        assert (S2[n2.index(f"high+{dy},{dx}")][3 + dy:9:3, 3 + dx:12:3] == 255 * rc.psum(h2)).all()
        assert (S2[n2.index(f"low+{dy},{dx}")][3 + dy:9:3, 3 + dx:12:3] == 255 * rc.nsum(h2)).all()


def test_tap_builders():
    for L, pos, neg, s in ((3, 248, 0, 0), (5, 100, 8, 0), (5, 33, 129, 3), (9, 32888, 0, 0), (5, 90, 1, 3)):
        h = rc.taps_1d(L, pos, neg, s)
        assert (rc.psum(h), -rc.nsum(h)) == (pos << s, neg << s) and rc.common_shift(h, 64) == s
    assert np.abs(rc.taps_1d(25, 526335, hmax=32639)).max() <= 32639
    for R in (3, 5):
        g = rc.taps_2d(R, R, 248, 9, 2)
        assert not rc.is_rank1(g) and rc.rank1_factor(g) is None and rc.common_shift(g, 64) == 2
        assert (rc.psum(g), -rc.nsum(g)) == (248 << 2, 9 << 2)
    o = rc.outer([1, -2, 1], [3, 5, 3])
    assert rc.is_rank1(o) and [v.tolist() for v in rc.rank1_factor(o)] == [[1, -2, 1], [3, 5, 3]]


def test_wide_threshold_and_its_model():
    """needs_wide (fir1d.hip:159-165) for int16 samples: sum|h| = 2^48 - 1 / 2^48.  x = -32768 under
    taps of one sign sums to 2^63 - 32768 / exactly 2^63 (Python ints).  The narrow form keeps the
    sum mod 2^64, sign-extended.  At acc_bits = 64 the reference's own wrap gives -2^63 too
    (conservative there); from acc_bits = 65 the narrow form differs on the rejected side only."""
    a, b = rc.wide_case()
    assert not rc.needs_wide(a, 64, 32768) and rc.needs_wide(b, 64, 32768)
    assert not rc.needs_wide(b, 63, 32768)  # a wrap to fewer than 64 bits is exact mod 2^64
    assert np.count_nonzero(a - b) == 1 and int(np.abs(a - b).max()) == 1
    sa = sum(int(v) * -32768 for v in a)
    sb = sum(int(v) * -32768 for v in b)
    assert (sa, sb) == ((1 << 63) - 32768, 1 << 63)

    def wrap(v, bits):
        return ((v + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1))

    for acc, differs in ((64, False), (65, True), (100, True)):
        assert wrap(wrap(sa, 64), acc) == wrap(sa, acc)
        assert (wrap(wrap(sb, 64), acc) != wrap(sb, acc)) is differs
    assert not rc.needs_wide(np.full(1 << 17, (1 << 31) - 1), 64, 255)  # u8: far from 2^63 (not covered)
