"""CPU: tests/fullrate_property_cases.py is right before tests/test_gpu_property_fullrate.py leans on it.

* every strategy, drawn DRAWS times under derandomized settings, yields a legal call (the Python
  restatement of check_fir1d / check_fir1d_ideal / check_fir2d / check_fir2d_ideal accepts it) at
  legal guard leads, within the sizes and the cost the issue sets;
* ``route_of`` with the tensors at the drawn leads equals the route the strategy intended, for
  every draw and every pinned example, and ``launches_of`` names the kernels of that route;
* over the draws of each family every route occurs, none under rate_property_cases.MIN_SHARE;
  PINNED holds every route;
* the draws hold what no single case shows: both sides of every tap-count edge, every fill, the
  halos present and absent, ragged and whole-vector images in one call, ...;
* ``want`` equals a direct Python-int loop over the definition (centre L // 2, zero padding or
  halos, mask to acc_bits and restore the sign, round half up, stage) at tiny sizes for the
  segment, bank and images families: the glue is right, not only the oracle;
* the limits the helper states are the constants of csrc, and ``route_of`` / ``launches_of`` agree
  with big_index_cases.dispatch_kernel on that module's small table.
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

import big_index_cases as bic
import fullrate_property_cases as fp
from rate_property_cases import MIN_SHARE, WORK

DRAWS = 1500
CSRC = Path(__file__).resolve().parents[1] / "warmup-fir-filter_amd" / "csrc"
FILLS = {"uniform", "ends", "min", "max"}


@functools.lru_cache(maxsize=None)
def _draws(fam: str) -> tuple:
    got = []

    @settings(max_examples=DRAWS, derandomize=True, database=None, deadline=None, phases=[Phase.generate],
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
    @given(fp.STRATEGIES[fam]())
    def collect(case):
        got.append(case)

    collect()
    return tuple(got)


def _lead_ok(lead: int, itemsize: int) -> bool:
    return 0 <= lead < 512 and lead % itemsize == 0  # what tests/guarded.py asks of lead_bytes


@pytest.mark.parametrize("fam", fp.FAMILIES)
def test_every_draw_is_a_legal_call(fam):
    cases = _draws(fam)
    assert len(cases) >= DRAWS * 2 // 3
    for c in cases + tuple(fp.PINNED[fam]):
        assert c.family == fam and c.route in fp.ROUTES[fam], c
        assert fp.check_sizes(c) is None, (fp.check_sizes(c), c)
        assert c.fill in FILLS and c.work <= (WORK * 6 if c in fp.TALL else WORK * 1.1), (c.work, c)
        in_size = 1 if fam in ("fir2d", "ideal") else c.in_itemsize
        if fam == "images":
            assert 0 <= len(c.images) <= 20 and 1 <= c.filters <= 8 and 1 <= c.taps <= 12, c
            for im in c.images:
                assert len(im.y_leads) == c.filters and _lead_ok(im.x_lead, in_size), c
                assert all(_lead_ok(y, c.out_itemsize) for y in im.y_leads), c
                assert 0 <= im.rows <= 12 and 0 <= im.width <= 5100, c
        else:
            assert _lead_ok(c.x_lead, in_size) and _lead_ok(c.y_lead, c.out_itemsize), c
            assert c.rows >= 1 and c.width >= 1 and c.frames in (0, 1, 2, 3), c
        if fam in ("rows", "bank"):
            assert c.rows <= 40 and 1 <= c.taps <= fp.MAX_LEN and c.ch in (1, 2, 3), c
        if fam == "segment":
            assert c.rows == 1 and len(c.halos) == 2 and _lead_ok(c.hl_lead, in_size) and _lead_ok(c.hr_lead, in_size), c
        if fam == "fir2d" and c not in fp.TALL:
            assert 1 <= len(c.hq) <= 7 and 1 <= len(c.hq[0]) <= 7 and c.rows <= 300 and c.width <= 1100, c
            assert c.path in (None, "reg", "mfma"), c
        x = fp.samples(replace(c, rows=min(c.rows, 2), width=min(c.width, 16)))
        first = x[0] if fam == "segment" else (x if fam != "images" else None)
        if first is not None:
            assert first.dtype == (np.uint8 if fam in ("fir2d", "ideal") else c.np_dtype), c


@pytest.mark.parametrize("fam", fp.FAMILIES)
def test_route_of_is_the_intended_route(fam):
    for c in _draws(fam) + tuple(fp.PINNED[fam]):
        assert fp.route_of(c) == c.route, (fp.route_of(c), c)
        ks = fp.launches_of(c)
        if fam == "rows":
            assert ks == [fp.GENERIC if c.route.startswith("generic") else {v: k for k, v in fp.ROWS_ROUTE.items()}[c.route]], c
        elif fam == "bank":
            assert len(ks) == (-(-c.filters // 4) if c.route == "fused" else c.filters), c
            assert c.route == "each" or set(ks) == {fp.REG}, c
        elif fam == "segment":
            bulk = fp.rows_kernel(c.u8, c.stage, c.ch, 1, c.width, c.hq, c.x_lead, c.y_lead, c.frac, c.acc)
            tail = {"one": [], "all_edge": [fp.GENERIC], "rows+edges": [fp.EDGES] if len(c.hq) > 1 else []}[c.route]
            assert ks == [fp.REG if c.route == "one" else bulk] + tail, c
        elif fam == "fir2d":
            assert ks == [fp.KERNEL_2D[c.route]], c
        elif fam == "ideal":
            assert ks == [fp.KERNEL_IDEAL[c.route]], c
        else:
            live = [im for im in c.images if im.rows * im.width]
            nb = sum(fp.image_batches(c, im, im.x_lead) for im in live)
            assert ks.count(fp.BATCH) == -(-nb // 8) * -(-c.filters // 4) and len(ks) - ks.count(fp.BATCH) == (len(live) - nb) * c.filters, c
            assert (c.route == "batch") == (nb == len(live) and (nb > 0 or fp.image_batches(c, fp.Image(1, 64), 0))), c


@pytest.mark.parametrize("fam", fp.FAMILIES)
def test_every_route_has_its_share(fam):
    cases = _draws(fam)
    seen = Counter(c.route for c in cases)
    share = {r: seen[r] / len(cases) for r in fp.ROUTES[fam]}
    print(fam, len(cases), {r: round(s, 3) for r, s in share.items()})
    assert set(seen) == set(fp.ROUTES[fam]), share
    assert min(share.values()) >= MIN_SHARE, share
    assert {c.route for c in fp.PINNED[fam]} == set(fp.ROUTES[fam])  # whatever is drawn, every route runs once


def _ks(L):
    return bic._mfma_ksteps(L)


@pytest.mark.parametrize("fam", fp.FAMILIES)
def test_draws_cover_what_the_issue_lists(fam):
    """Properties of the whole set of draws that no single case shows."""
    cases = _draws(fam)
    assert {c.fill for c in cases} == FILLS
    if fam in ("rows", "segment", "bank", "images"):
        assert {c.stage for c in cases} == {fp.U8, fp.I32} and {c.dtype for c in cases} == {"u8", "i16"}
        assert {c.ch for c in cases} == {1, 2, 3}
        assert any(c.frac >= 32 for c in cases) and any(c.acc > 32 for c in cases) and any(c.acc < 32 for c in cases)
        flat = [np.asarray(c.hq, dtype=object).reshape(-1) for c in cases]
        assert any(max(abs(int(v)) for v in h) > 1 << 23 for h in flat)
    if fam == "rows":
        lens = {c.taps for c in cases}
        assert lens >= {1, 9, 10, 39, 40, 64, 65, 66} and max(lens) >= 2000
        for k in (3, 8, 12, 16, 24, 32, 48):  # both sides of every k-step edge, by either kernel's count
            assert {k, k + 1} <= {_ks(L) for L in lens} and {k, k + 1} <= {fp._mfma_ksteps16(L) for L in lens}, k
        for r, lo, hi in (("mfma_run", 17, 32), ("mfma_run", 33, 48), ("mfma_long", 17, 32), ("mfma_long", 33, 48)):
            assert any(c.route == r and lo <= _ks(c.taps) <= hi for c in cases), (r, lo)  # two and three chunks
        assert any(c.route == "mfma_step" and 32639 in c.hq for c in cases) and any(c.route == "lds" and 32640 in c.hq for c in cases)
        assert any(32768 in c.hq for c in cases) and any(-32769 in c.hq for c in cases)
        assert any(c.rows == 1 for c in cases) and any(c.rows > 30 for c in cases)
        for u8, vec, tile in ((True, 16, 4096), (False, 8, 512)):
            widths = {c.width * c.ch for c in cases if c.u8 == u8}
            assert min(widths) <= 2 and vec in widths and {vec - 1, vec + 1} & widths, u8
            assert any(abs(w - tile) <= vec for w in widths) and any(abs(w - 1024) <= 8 for w in widths) and max(widths) > 2 * tile
        reg = [c for c in cases if c.route == "reg" and c.rows > 1]
        need = lambda c: (16 if c.u8 else 8) + (c.taps - 1) * c.ch  # noqa: E731
        assert any(c.width * c.ch == need(c) for c in reg)  # the shortest row the register kernel takes ...
        assert any(c.route == "generic:shape" and c.taps <= 9 and c.width * c.ch == need(c) - 1 for c in cases)  # ... and one less
        assert {c.x_lead % 16 for c in cases} >= {0, 8, 1} and any(c.y_lead % 2 for c in cases)
    if fam == "segment":
        assert {c.halos for c in cases} == {(a, b) for a in (True, False) for b in (True, False)}
        assert any(sum(c.halo_sizes) > 500 for c in cases if c.route == "rows+edges")  # halos hundreds of samples long
        assert any(c.width == 1 for c in cases)
        assert any(c.width * c.ch == sum(c.halo_sizes) for c in cases)
        bulk = {fp.launches_of(c)[0] for c in cases if c.route == "rows+edges"}
        assert bulk == {fp.REG, fp.STEP, fp.RUN, fp.LONG, fp.LDS, fp.GENERIC}
        assert any(c.route == "rows+edges" and c.taps <= 9 and abs(c.width * c.ch - (4096 if c.u8 else 512)) == c.ch for c in cases)
    if fam == "bank":
        assert {c.filters for c in cases} == set(range(1, 9))
        each = {k for c in cases if c.route == "each" for k in fp.launches_of(c)}
        assert each >= {fp.REG, fp.LDS, fp.GENERIC, fp.STEP}, each
        assert any(c.route == "fused" and c.y_lead % 2 for c in cases)
    if fam == "images":
        assert {len(c.images) for c in cases} >= {0, 1, 8, 9, 20} and {c.filters for c in cases} == set(range(1, 9))
        assert {c.taps for c in cases} == set(range(1, 13))
        ims = [im for c in cases for im in c.images]
        assert any(im.rows == 0 for im in ims) and any(im.width == 0 for im in ims)
        assert any(im.rows == 1 and 0 < im.width < 16 for im in ims)
        assert any(y % 2 for im in ims for y in im.y_leads)
        assert any(im.x_lead % 16 for im in ims)
        batch = [[im for im in c.images if im.rows * im.width and fp.image_batches(c, im, im.x_lead)] for c in cases]
        assert any(len(b) > 8 for b in batch)  # several launches
        assert any({im.width % 16 == 0 or im.rows == 1 for im in b} == {True, False} for b in batch)  # ragged and whole-vector rows
        assert any(all(im.width % 16 == 0 or im.rows == 1 for im in b) and len(b) > 1 for b in batch)  # no ragged image: no kDefer
    if fam == "fir2d":
        assert {len(c.hq) for c in cases} == {len(c.hq[0]) for c in cases} == set(range(1, 8))
        assert {c.path for c in cases} == {None, "reg", "mfma"} and {c.frames for c in cases} == {0, 1, 2, 3}
        assert {c.stage for c in cases} == {fp.U8, fp.I32}
        widths = {c.width for c in cases}
        assert {1008, 1024, 1040} <= widths and any(w % 16 for w in widths) and max(c.rows for c in cases) > 250
        for route in ("mfma", "reg", "generic"):
            assert {c.path for c in cases if c.route == route} == {None, "reg", "mfma"} - ({"reg"} if route == "mfma" else set()), route
        assert [c.rows for c in fp.TALL] == [65535 * 16, 65535 * 16 + 1] and [c.route for c in fp.TALL] == ["reg", "generic"]
        assert all(c.width == 16 and (len(c.hq), len(c.hq[0])) == (3, 3) and fp.rg.is_rank1(c.hq) for c in fp.TALL)
    if fam == "ideal":
        assert any(c.frames for c in cases) and any(c.rows > 1 and c.route == "1d:reg" for c in cases)


# ---- the references against the definition ------------------------------------------------------------
def _loop(x, hq, frac, acc, stage, ch, hl=None, hr=None):
    """One row as plain Python ints from the definition; hl / hr: the samples before and after it."""
    n, L = len(x) // ch, len(hq)
    c = L // 2
    nl, nr = L - 1 - c, c
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)
    out = np.zeros(n * ch, np.uint8 if stage == fp.U8 else np.int32)
    for q in range(ch):
        for j in range(n):
            s = 0
            for k in range(L):
                i = j - k + c
                if 0 <= i < n:
                    v = int(x[i * ch + q])
                elif i < 0:
                    v = int(hl[(nl + i) * ch + q]) if hl is not None else 0
                else:
                    v = int(hr[(i - n) * ch + q]) if hr is not None else 0
                s += int(hq[k]) * v
            s &= mask
            if s & sign:
                s -= 1 << acc
            v = (s + bias) >> frac
            if stage == fp.U8:
                v = 0 if v < 0 else (255 if v > 255 else v)
            else:
                v = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the int32 stage keeps the low 32 bits
            out[j * ch + q] = v
    return out


@pytest.mark.parametrize("fam", ["segment", "bank", "images"])
def test_references_equal_a_direct_loop_at_tiny_sizes(fam):
    cases = _draws(fam)
    picked = [fp.smaller(c) for c in cases[:: len(cases) // 16][:16]] + [fp.smaller(c) for c in fp.PINNED[fam]]
    halos = set()
    for c in picked:
        x = fp.samples(c)
        ref = fp.want(c, x)
        if fam == "segment":
            xs, hl, hr = x
            halos.add((hl is not None, hr is not None))
            assert ref.shape == xs.shape and np.array_equal(ref, _loop(xs, c.hq, c.frac, c.acc, c.stage, c.ch, hl, hr)), c
            continue
        for xi, ri in zip(x if fam == "images" else [x], ref if fam == "images" else [ref]):
            assert ri.shape == (c.filters,) + xi.shape, c
            for f, h in enumerate(c.hq):
                for r in range(xi.shape[0]):
                    assert np.array_equal(ri[f, r], _loop(xi[r], h, c.frac, c.acc, c.stage, c.ch)), (c, f, r)
    assert fam != "segment" or len(halos) == 4
    if fam == "images":  # the second launch of a plan sees other samples of the same shapes
        c = fp.PINNED["images"][0]
        a, b = fp.samples(c), fp.samples(c, again=1)
        assert [v.shape for v in a] == [v.shape for v in b] and any(not np.array_equal(u, v) for u, v in zip(a, b))


def test_a_mismatch_is_described_in_the_outputs_coordinates():
    c = fp.PINNED["rows"][3]  # int16, two channels
    ref = fp.want(c, fp.samples(c))
    assert fp.describe_mismatch(c, ref.copy(), ref) is None
    got = ref.copy()
    got[1, 9] += 1
    text = fp.describe_mismatch(c, got, ref)
    assert "row 1, sample 9 (frame 4, channel 1)" in text and "[reg]" in text and f"got {got[1, 9]!r}, want {ref[1, 9]!r}" in text
    assert "want (2, 24)" in fp.describe_mismatch(c, got[:, :-2], ref)
    c = fp.PINNED["ideal"][0]
    ref = fp.want(c, fp.samples(c))
    got = ref.copy()
    got[2, 1] = -got[2, 1] if got[2, 1] else -0.0  # a flipped sign bit alone is a difference
    assert "row 2, sample 1" in fp.describe_mismatch(c, got, ref).replace("column", "sample")
    zero = np.zeros((1, 4))
    assert fp.describe_mismatch(c, -zero, zero) is not None and fp.describe_mismatch(c, zero.copy(), zero) is None


# ---- the restatements against the sources and against big_index_cases --------------------------------
def test_the_limits_are_the_sources():
    for name, (file, value) in fp.LIMITS.items():
        m = re.search(rf"constexpr int [^;]*\b{name} = (\d+)[,;]", (CSRC / file).read_text())
        assert m and int(m.group(1)) == value, (name, file)
    lim = {k: v for k, (_, v) in fp.LIMITS.items()}
    assert (fp.MFMA_MIN, fp.MFMA_MIN_I32, fp.LDS_MAX_TAPS, fp.LDS_VEC) == (lim["kMfmaMinTaps"], lim["kMfmaMinTapsI32"], lim["kLdsMaxTaps"], lim["kLdsVec"])
    assert (fp.MF_TILE, fp.MF_MAX_TAPS, fp.REG_BATCH) == (lim["kMfTile"], lim["kMfMaxTaps"], lim["kRegBatch"])
    assert (fp.VEC2D, fp.STRIP2D, fp.IDEAL2D_MAX) == (lim["kVec2d"], lim["kStrip2dSep"], lim["kIdeal2dMaxRC"])
    assert fp.TALL_H == 65535 * lim["kStrip2dSep"] and lim["kMf2Blocks"] * lim["kBlock"] // lim["kWave"] == 2048 * 4
    text = {f: (CSRC / f).read_text() for f in ("fir1d.hip", "fir2d.hip", "ideal.hip", "ideal2d.hip", "fir1d_mfma.hip", "fir2d_mfma.hip")}
    for file, line in (("fir1d.hip", "return L <= 9 && (ch == 1 || (ch == 2 && in_dtype == FIR_IN_I16))"),
                       ("fir1d.hip", "if (total <= hle + hre) {"), ("fir1d.hip", "total % reg_tile_samples(in_dtype == FIR_IN_U8) == 0"),
                       ("fir2d.hip", "H <= 65535 * (int64_t)kStrip2dSep"), ("fir2d.hip", "(R == 1 || R == 3 || R == 5) && (C == 1 || C == 3 || C == 5)"),
                       ("fir2d_mfma.hip", "FIR2D_M2(3) FIR2D_M2(5)"), ("fir2d_mfma.hip", "if (v < -32768 || v > 32639) return 0;"),
                       ("fir1d_mfma.hip", "taps_ok &= hq[k] >= -32768 && hq[k] <= 32639;"), ("fir1d_mfma.hip", "if (KS > 3) {"),
                       ("ideal.hip", "const bool reg = L <= 9 &&"), ("ideal2d.hip", "W % 4 == 0 && W >= 4 + C - 1")):
        assert line in text[file], (file, line)
    assert fp.REG_MAX_TAPS == 9 and fp._mfma_ksteps(65) == 3 and fp._mfma_ksteps(66) == 4 and bic._mfma_ksteps is fp._mfma_ksteps


def test_route_of_agrees_with_the_big_index_dispatcher():
    """dispatch_kernel's ``fixed``, ``bank`` and ``ideal`` branches are this module's functions; on
    big_index_cases.table(SMALL) the Case-level route_of / launches_of say the same."""
    seen = set()
    for b in bic.table(bic.SMALL):
        if b.family not in ("fixed", "bank", "ideal"):
            continue
        for x_ptr, y_ptr in ((4096 + b.x_off * b.in_itemsize, 8192), (4096, 8192), (4096 + 8, 8192), (4096, 8192 + 8), (4097, 8192)):
            if x_ptr % b.in_itemsize or (b.family == "bank" and (x_ptr, y_ptr) != (4096, 8192)):
                continue
            kernel = bic.dispatch_kernel(b, x_ptr, y_ptr)
            h = bic.taps_of(b)
            if b.family == "ideal":
                c = fp.Case("ideal", "1d:reg", hq=tuple(float(v) for v in h), rows=b.rows, width=b.width)
                assert fp.launches_of(c, x_ptr, y_ptr) == [kernel] and fp.KERNEL_IDEAL[fp.route_of(c, x_ptr, y_ptr)] == kernel, b
            elif b.family == "bank":
                c = fp.Case("bank", "fused", b.dtype, b.ch, b.stage, tuple(tuple(int(v) for v in r) for r in h), bic.FRAC, bic.ACC, b.rows, b.width)
                assert fp.route_of(c, x_ptr, y_ptr) == "fused" and set(fp.launches_of(c, x_ptr, y_ptr)) == {kernel}, b
            else:
                c = fp.Case("rows", "reg", b.dtype, b.ch, b.stage, tuple(int(v) for v in h), bic.FRAC, bic.ACC, b.rows, b.width)
                assert fp.launches_of(c, x_ptr, y_ptr) == [kernel], b
                route = fp.route_of(c, x_ptr, y_ptr)
                assert fp.ROWS_ROUTE.get(kernel, "generic") == route.split(":")[0], (b, route)
            seen.add(kernel)
    assert seen >= {fp.REG, fp.STEP, fp.RUN, fp.LONG, fp.LDS, fp.GENERIC, "fir1d_ideal_reg_kernel", "fir1d_ideal_kernel"}
