"""CPU: tests/rate_property_cases.py is right before tests/test_gpu_property_rate.py leans on it.

* every strategy, drawn DRAWS times under derandomized settings, yields a legal call (the Python
  restatement of check_fir1d_*'s size rules accepts it; the library's pure *_out_width agrees with
  the shape the reference's stuffing and slicing give), at legal guard leads;
* ``route_of`` with x and y at the drawn leads equals the route the strategy intended, for every
  draw and every pinned example;
* over the draws of each family every route occurs, none under MIN_SHARE, ``fast`` inside
  FAST_SHARE (conditions chosen from the strategies' weights, see the helper);
* the references equal a direct Python-int loop over the definition (zero-stuff by U, filter with
  centre L // 2 and zero padding, mask to acc_bits and restore the sign, round half up, stage, keep
  every D-th frame from ``phase``) at tiny sizes: the stuffing and slicing glue is right, not
  only the oracle;
* the limits the helper states are the constants of the four .hip files.
"""
from __future__ import annotations

import functools
import re
from collections import Counter
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest
from hypothesis import HealthCheck, Phase, given, settings

import rate_property_cases as rc
from cplx_ref import cplx_loop

DRAWS = 1500
CSRC = Path(__file__).resolve().parents[1] / "warmup-fir-filter_amd" / "csrc"


@functools.lru_cache(maxsize=None)
def _draws(fam: str) -> tuple:
    got = []

    @settings(max_examples=DRAWS, derandomize=True, database=None, deadline=None, phases=[Phase.generate],
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
    @given(rc.STRATEGIES[fam]())
    def collect(case):
        got.append(case)

    collect()
    return tuple(got)


def _lead_ok(lead: int, itemsize: int) -> bool:
    return 0 <= lead < 512 and lead % itemsize == 0  # what tests/guarded.py asks of lead_bytes


def _ref_shape(c: rc.Case) -> tuple:
    """The shape the reference's glue gives: the stuffed row sliced [:, phase::D], no oracle run."""
    return np.empty((c.rows, c.width * c.up, c.ch), np.uint8)[:, c.phase::c.decim].reshape(c.rows, -1).shape


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_every_draw_is_a_legal_call(fam):
    cases = _draws(fam)
    assert len(cases) >= DRAWS * 2 // 3
    for c in cases + tuple(rc.PINNED[fam]):
        assert c.family == fam and c.route in rc.ROUTES[fam], c
        assert rc.check_sizes(c) is None, (rc.check_sizes(c), c)
        assert 1 <= c.rows <= 12 and 1 <= c.width <= rc.MAX_WIDTH[fam] + 3, c
        assert c.fill in ("uniform", "ends", "min", "max"), c
        assert _lead_ok(c.x_lead, 1 if c.dtype == "u8" else 2) and _lead_ok(c.y_lead, c.out_itemsize), c
        assert _ref_shape(c) == (c.rows, rc.out_width(c) * c.ch), c
        if fam == "cplx":
            assert (c.dtype, c.ch, c.up, c.decim, c.phase) == ("i16", 2, 1, 1, 0), c
        x = rc.samples(replace(c, rows=min(c.rows, 2), width=min(c.width, 16)))
        assert x.dtype == c.np_dtype and x.shape == (min(c.rows, 2), min(c.width, 16) * c.ch), c


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_route_of_is_the_intended_route(fam):
    for c in _draws(fam) + tuple(rc.PINNED[fam]):
        assert rc.route_of(c, c.x_lead, c.y_lead) == c.route, c
        assert (rc.forwarded_to(c) is not None) == (c.route == "forward"), c


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_every_route_has_its_share(fam):
    cases = _draws(fam)
    seen = Counter(c.route for c in cases)
    share = {r: seen[r] / len(cases) for r in rc.ROUTES[fam]}
    print(fam, len(cases), {r: round(s, 3) for r, s in share.items()})
    assert set(seen) == set(rc.ROUTES[fam]), share
    assert min(share.values()) >= rc.MIN_SHARE, share
    assert rc.FAST_SHARE[0] <= share["fast"] <= rc.FAST_SHARE[1], share
    assert {c.route for c in rc.PINNED[fam]} == set(rc.ROUTES[fam])  # whatever is drawn, every route runs once


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_draws_cover_what_the_issue_lists(fam):
    """Properties of the whole set of draws that no single case shows."""
    cases = _draws(fam)
    assert {c.fill for c in cases} == {"uniform", "ends", "min", "max"}
    assert any(c.rows == 1 for c in cases) and any(c.rows > 1 for c in cases)
    assert any(c.frac >= 32 for c in cases) and any(c.acc > 32 for c in cases) and any(c.acc < 32 for c in cases)
    flat = [np.asarray(c.hq, dtype=object).reshape(-1) for c in cases]
    assert any((h == 0).any() for h in flat) and any(max(abs(int(v)) for v in h) > 1 << 23 for h in flat)
    if fam == "cplx":
        assert any(c.taps > rc.MAX_TAPS_CPLX for c in cases) and any(c.taps == rc.MAX_TAPS_CPLX for c in cases)
        assert any(c.rows > 1 and c.width % 4 == 2 for c in cases)
        assert any(c.route == "fast" and c.width > 1024 for c in cases)
        return
    assert {c.stage for c in cases} == {rc.U8, rc.I32}
    assert {(c.dtype, c.ch) for c in cases} >= {("u8", 1), ("i16", 1), ("i16", 2), ("i16", 3), ("u8", 2)}
    assert any(c.y_lead % 16 for c in cases if c.route == "fast")
    rate = (lambda c: c.decim) if fam == "decim" else (lambda c: c.up)
    rates = {rate(c) for c in cases}
    assert rates >= {1, 2, 16, 17} and len(rates & set(range(2, 17))) >= 12 and max(rates) > 24
    assert any(c.taps > 128 for c in cases)
    if fam != "interp":
        assert any(c.phase == c.decim - 1 and c.decim > 1 for c in cases) and any(c.width < c.decim for c in cases)
    if fam != "decim":
        assert any(c.taps < c.up for c in cases) and any(c.taps % c.up for c in cases)  # phases with no tap, uneven phases
        assert any(c.up > 1 and not any(c.hq[p::c.up]) for c in cases for p in range(min(c.up, c.taps)))  # an all-zero phase
    if fam == "resample":
        fast = {(c.up, c.decim) for c in cases if c.route == "fast"}
        assert any(np.gcd(u, d) == 1 for u, d in fast) and any(1 < np.gcd(u, d) < min(u, d) for u, d in fast)
        assert any(d % u == 0 and d > u for u, d in fast) and any(u % d == 0 and u > d for u, d in fast)
        assert {rc.forwarded_to(c) for c in cases if c.route == "forward"} == {"decim", "interp"}


# ---- the references against the definition ------------------------------------------------------------
def _loop(x, hq, U, D, phase, frac, acc, stage, ch):
    """Zero-stuff by U, filter, keep [phase::D], as plain Python ints from the definition."""
    rows, width = x.shape[0], x.shape[1] // ch
    hs, L = [int(v) for v in hq], len(hq)
    c, mid = L // 2, width * U
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)
    kept = range(phase, mid, D)
    out = np.zeros((rows, len(kept) * ch), np.uint8 if stage == rc.U8 else np.int32)
    for r in range(rows):
        for q in range(ch):
            for m, j in enumerate(kept):
                s = 0
                for k in range(L):
                    i = j - k + c  # a frame of the stuffed row: zero unless it is a multiple of U inside the row
                    if 0 <= i < mid and i % U == 0:
                        s += hs[k] * int(x[r, (i // U) * ch + q])
                s &= mask
                if s & sign:
                    s -= 1 << acc
                v = (s + bias) >> frac
                if stage == rc.U8:
                    v = 0 if v < 0 else (255 if v > 255 else v)
                else:
                    v = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the int32 stage keeps the low 32 bits
                out[r, m * ch + q] = v
    return out


def _tiny(c: rc.Case) -> rc.Case:
    """The case cut down to a few taps and frames (its route no longer matters here)."""
    n = 4 if c.family == "cplx" else 7
    return replace(c, rows=min(c.rows, 2), width=min(c.width, 11), hq=c.hq[:n])


@pytest.mark.parametrize("fam", rc.FAMILIES)
def test_references_equal_a_direct_loop_at_tiny_sizes(fam):
    cases = _draws(fam)
    picked = [_tiny(c) for c in cases[:: len(cases) // 12][:12]] + [_tiny(c) for c in rc.PINNED[fam][-2:]]
    for c in picked:
        x = rc.samples(c)
        ref = rc.want(c, x)
        if fam == "cplx":
            loop = cplx_loop(x, c.hq, c.frac, c.acc, c.stage)
        else:
            loop = _loop(x, c.hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch)
        assert ref.shape == loop.shape == (c.rows, rc.out_width(c) * c.ch) and ref.dtype == loop.dtype, c
        assert np.array_equal(ref, loop), (c, np.argwhere(ref != loop)[:4].tolist())


def test_a_mismatch_is_described_in_the_grids_words():
    c = rc.PINNED["resample"][-2]
    ref = rc.want(c, rc.samples(c))
    assert rc.describe_mismatch(c, ref.copy(), ref) is None
    got = ref.copy()
    got[2, 9] += 1
    text = rc.describe_mismatch(c, got, ref)
    assert "row 2, output frame 9 (period 1, q 2, frame 119 of the interpolated row)" in text and "[fast]" in text
    assert f"got {got[2, 9]}, want {ref[2, 9]}" in text
    c = rc.PINNED["cplx"][0]
    ref = np.zeros((2, 2 * 1028), np.int32)
    got = ref.copy()
    got[1, 7] = 5
    assert "row 1, frame 3 (im): got 5, want 0" in rc.describe_mismatch(c, got, ref)
    assert "want (2, 2056)" in rc.describe_mismatch(c, got[:, :-2], ref)


def test_the_limits_are_the_sources():
    for name, (file, value) in rc.LIMITS.items():
        m = re.search(rf"constexpr int {name} = (\d+);", (CSRC / file).read_text())
        assert m and int(m.group(1)) == value, (name, file)
    assert rc.MAX_RATE == rc.LIMITS["kDecMaxD"][1] == rc.LIMITS["kIntMaxU"][1] == rc.LIMITS["kResMaxUD"][1]
    assert rc.MAX_TAPS_REAL == rc.LIMITS["kDecMaxTaps"][1] == rc.LIMITS["kIntMaxTaps"][1]
    assert rc.MAX_PHASE_TAPS == rc.LIMITS["kResMaxPhaseTaps"][1] and rc.MAX_TAPS_CPLX == rc.LIMITS["kCxMaxTaps"][1]
    assert rc.CPLX_VEC == rc.LIMITS["kCxVec"][1]
