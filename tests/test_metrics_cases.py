"""CPU: tests/metrics_cases.py is right before tests/test_gpu_metrics_forms.py leans on it.

* its constants are those of csrc/metrics.hip and fir_common.h, read back from the sources, and the
  lines of launch_metrics_t that ``part_bounds`` / ``launches_of`` restate stand there verbatim;
* ``sums_ref`` ties to the oracle: fir_hip.metrics_from_sums of it equals
  oracle.fir_oracle.compute_metrics bit for bit on small cases of every dtype;
* the periodic reference equals ``sums_ref`` of the materialised tiled array at about a thousand
  blocks with a ragged tail (and below one period), for all eight values;
* the pattern's 509 block sums are pairwise distinct in each of the three arrays;
* for every pinned size, every mutant order (``metrics_cases.mutants``) gives another sum d than the
  reference; which of them sum|d| and sum d^2 see is printed (``-s``), not demanded: all-positive
  sums absorb an early difference.  The three arrays' references differ from each other, so a
  chain that reads another array's block sums shows in all three;
* the pinned table reaches what it names (parts, grids, the last Cnt slot), and the property
  test's strategy, drawn under the GPU test's own settings, yields every route, every dtype, every
  fill and the size edges, each a legal call that ``launches_of`` sends where the route says.
"""
from __future__ import annotations

import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
from hypothesis import HealthCheck, Phase, given, settings

import fir_hip
import metrics_cases as mc
from conftest import load_metrics_dtypes, same_metrics
from oracle import fir_oracle as fo

CSRC = Path(__file__).resolve().parents[1] / "warmup-fir-filter_amd" / "csrc"


def test_the_constants_are_the_sources():
    text = (CSRC / "metrics.hip").read_text() + (CSRC / "fir_common.h").read_text()
    for name, value in mc.CONSTANTS.items():
        m = re.search(rf"constexpr (?:int|int64_t) {name} = (\d+);", text)
        assert m and int(m.group(1)) == value, name
    for line in ("const bool vec = (uintptr_t)ideal % 16 == 0 && (uintptr_t)fixed % 16 == 0;",
                 "if (vec && nbf > 0) {",
                 "const int g = (int)(want > kMetricPBlocks ? kMetricPBlocks : want);",
                 "dim3(kMetricPrepBlocks)", "dim3(g + 1)",
                 "const int64_t want = nparts == 0 ? kTailPart : kBodyPart;",
                 "const int64_t take = nparts == kMaxParts - 1 || left <= want ? left : want;",
                 "bounds[q + 1] = bounds[q] + sizes[nparts - 1 - q];",
                 "const int64_t want = (hi - lo + kBlock / kWave - 1) / (kBlock / kWave);",
                 "const int g = (int)(want > kMetricBlocks ? kMetricBlocks : want);",
                 "const unsigned grid = (unsigned)g + (prev_hi > prev_lo ? 1u : 0u);",
                 "if (nb > nbf) {",
                 "constexpr int64_t kCntSlots = (int64_t)kMaxParts * kMetricBlocks + 1;",
                 "constexpr int kChainGS = kChainDepth * kWave;",
                 "return sizeof(Cnt) * kCntSlots + 64 + 3 * sizeof(double) * (size_t)metrics_nblocks(n);"):
        assert line in text, line
    assert (mc.WAVES, mc.GROUP, mc.CNT_SLOTS) == (4, 512, 8193)
    assert set(mc.TARG) == {np.dtype(d).name for d in fir_hip.METRIC_DTYPES}


def _small_cases():
    rng = np.random.default_rng(5)
    for name, yi, yf, _ in load_metrics_dtypes():
        yield name, yi, yf
    for dtype in mc.ALL_DTYPES:
        for i, n in enumerate((1, 7, 100, 8192 + 129, 2 * 8192)):
            for fill in ("spread", "image", "exact:-0"):
                c = mc.Case("x", dtype, dtype, n // mc.PW, n % mc.PW, 0, 0, fill, int(rng.integers(1 << 20)) + i)
                yield f"{dtype}-{n}-{fill}", *mc.make_data(c)


def test_sums_ref_ties_to_the_oracle():
    seen = 0
    for name, yi, yf in _small_cases():
        with np.errstate(invalid="ignore"):  # (the golden cases hold NaN and infinities)
            s = mc.sums_ref(yi, yf)
            got, want = fir_hip.metrics_from_sums(np.append(s, 0.0), yi.size), fo.compute_metrics(yi, yf)
        assert not same_metrics(got, want), (name, {k: (got[k], want[k]) for k in same_metrics(got, want)})
        assert s[7] == yi.size and s.shape == (8,)
        seen += 1
    assert seen > 150
    e = mc.sums_ref(np.zeros(0), np.zeros(0, np.uint8))
    assert not mc.differing(e, np.zeros(8)) and fir_hip.metrics_from_sums(np.append(e, 0.0), 0) == fo.compute_metrics(np.zeros(0), np.zeros(0, np.uint8))
    nan = mc.sums_ref(np.array([1.0, np.nan, 3.0]), np.array([0, 255, 7], np.uint8))
    assert np.isnan(nan[0]) and np.isnan(nan[1]) and list(nan[4:]) == [1, 1, 0, 3]  # np.max propagates NaN


def test_differing_sees_the_sign_of_zero_and_takes_nan_for_nan():
    a = np.array([0.0, np.nan, 1.0, -0.0])
    assert mc.differing(a, a.copy()) == []
    assert mc.differing(a, np.array([-0.0, np.nan, np.nextafter(1.0, 2.0), -0.0])) == [0, 2]
    assert "out[2]" in mc.describe(a, np.array([0.0, np.nan, 2.0, -0.0]))


def test_launches_of_on_the_pinned_table():
    assert [(r.nbf, r.m) for r in mc.ROWS] == [(2048, 0), (2049, 1), (2048 + 513, 129), (2048 + 2049, 4321),
                                               (2048 + 8192, 0), (2048 + 8192 + 1, 7), (2048 + 14 * 8192 + 8193, 4321)]
    bounds = [mc.part_bounds(r.nbf) for r in mc.ROWS]
    assert bounds[:6] == [[0, 2048], [0, 1, 2049], [0, 513, 2561], [0, 2049, 4097], [0, 8192, 10240], [0, 1, 8193, 10241]]
    assert len(bounds[6]) == 17 and bounds[6][1] == 8193 and bounds[6][-1] - bounds[6][-2] == 2048
    assert all(b - a == 8192 for a, b in zip(bounds[6][1:-2], bounds[6][2:-1]))
    A = 1 << 20  # a 16-byte aligned address
    mb, sh = lambda g: ("metrics_blocks", (), g), lambda g: ("metrics_blocks_any", ("short",), g)  # noqa: E731
    fin, rag8, rag16 = ("metrics_final", (), 1), ("metrics_ragged", ("unsigned char",), 1), ("metrics_ragged", ("short",), 1)
    r = mc.ROWS
    assert mc.launches_of(r[0].n, "uint8", A, A + 1) == [mb(512), fin]
    assert mc.launches_of(r[1].n, "uint8", A, A + 1) == [mb(1), mb(513), rag8, fin]
    assert mc.launches_of(r[2].n, "int16", A, A) == [sh(129), sh(513), rag16, fin]
    assert mc.launches_of(r[3].n, "uint8", A + 8, A) == [mb(512), mb(513), rag8, fin]  # 2049 blocks: g capped
    assert mc.launches_of(r[4].n, "int16", A, A) == [sh(512), sh(513), fin]
    assert mc.launches_of(r[5].n, "uint8", A, A + 1) == [mb(1), mb(513), mb(513), rag8, fin]
    assert mc.launches_of(r[6].n, "int16", A, A) == [sh(512)] + [sh(513)] * 15 + [rag16, fin]
    assert mc.cnt_slots_used(r[6].n) == mc.CNT_SLOTS and mc.cnt_slots_used(r[6].n - 1) == mc.CNT_SLOTS
    assert mc.cnt_slots_used((2048 + 14 * 8192 + 2044) * mc.PW + 1) == mc.CNT_SLOTS - 1  # a first part under 512 workgroups
    for row in r:  # the twin: one launch, whatever the size
        g = min(256, -(-row.nbf // 4)) + 1
        assert mc.launches_of(row.n, "uint8", A, A) == [("metrics_prep", ("unsigned char",), 64), ("metrics_leaf_kernel", (), g)]
    assert mc.launches_of(0, "float64", A, A) == [fin] and mc.launches_of(5, "bool", A, A) == [rag8, fin]
    assert mc.launches_of(8192, "bool", A, A)[1][0] == "metrics_leaf_kernel" and mc.launches_of(8192, "int8", A, A)[0] == ("metrics_blocks_any", ("signed char",), 1)
    assert len(mc.pinned_cases()) == 7 * 2 + 4 * 2 and all(f.every_row or row.nbf <= 4097 for row, f in mc.pinned_cases())
    # each row is the smallest n that reaches what it names: one block or one sample less does not
    assert len(mc.part_bounds(2048)) == 2 and len(mc.part_bounds(2049)) == 3 and len(mc.part_bounds(2048 + 8192)) == 3
    assert len(mc.part_bounds(2048 + 8192 + 1)) == 4 and len(mc.part_bounds(2048 + 14 * 8192 + 8192)) == 17
    assert mc.part_bounds(2048 + 14 * 8192 + 8192)[1] == 8192  # ... but its first part is no larger than a body part


def test_the_pattern_block_sums_are_pairwise_distinct():
    pb = mc.pattern_blocks()
    for a in range(3):
        assert len(set(pb.sums[a].tolist())) == mc.P, a
    yi, yf = mc.pattern()
    d = yf.astype(np.float64) - yi
    assert (d < 0).sum() > mc.P * mc.PW // 3 and (d > 0).sum() > mc.P * mc.PW // 3
    mag = np.abs(d[d != 0])
    assert mag.min() < 2.0 ** -30 and 2.0 ** 30 < mag.max() < 2.0 ** 41
    assert abs(mc.chain(pb.sums[2])) < 1.0  # the pattern's sum d: the tiled sum does not drift


@pytest.mark.parametrize("n", [1021 * mc.PW + 4321, 2 * mc.P * mc.PW, 100 * mc.PW + 7, 4321])
def test_the_periodic_reference_equals_numpy_on_the_materialised_array(n):
    want = mc.sums_ref(*mc.tiled(n))
    got = mc.periodic_ref(n)
    assert not mc.differing(got, want), mc.describe(got, want)
    seq, r = mc.block_seq(n)
    assert seq.shape == (3, n // mc.PW) and (r is None) == (n % mc.PW == 0)


KINDS = ("reset", "parts_reversed", "groups_swapped", "dropped", "repeated", "ragged_first")


@pytest.mark.parametrize("row", mc.ROWS, ids=[r.id for r in mc.ROWS])
def test_every_mutant_order_changes_sum_d(row):
    seq, r = mc.block_seq(row.n)
    bounds = mc.part_bounds(row.nbf)
    ref = mc.periodic_ref(row.n)[1:4]
    assert len({float(v) for v in ref}) == 3  # a chain on another array's block sums differs in all three
    seen = {a: dict(mc.mutants(seq[a], None if r is None else r[a], bounds)) for a in range(3)}
    same_d = [k for k, v in seen[2].items() if v == ref[2]]
    assert not same_d, same_d
    kinds = Counter(k.split("@")[0] for k in seen[2])
    want = {"groups_swapped"} | ({"reset", "parts_reversed", "dropped", "repeated"} if len(bounds) > 2 else set()) | ({"ragged_first"} if row.m else set())
    assert set(kinds) == want, kinds
    for a, name in ((0, "sum|d|"), (1, "sum d^2")):
        blind = [k for k, v in seen[a].items() if v == ref[a]]
        print(f"{row.id}: {len(seen[a])} mutants, {name} unchanged by {len(blind)}: {blind[:8]}")


def test_the_mutants_are_what_they_say():
    seq = np.arange(1.0, 2049.0 + 1024.0)  # exact integer sums: 3072 blocks in parts [0, 1024), [1024, 3072)
    total = float(seq.sum())
    got = dict(mc.mutants(seq, 0.5, [0, 1024, 3072]))
    assert got["reset@1024"] == total - float(seq[:1024].sum()) + 0.5
    assert got["parts_reversed"] == got["ragged_first"] == got["groups_swapped@0"] == total + 0.5  # exact sums: any order
    assert got["dropped@1023"] == total - 1024.0 + 0.5 and got["repeated@1024"] == total + 1025.0 + 0.5
    assert set(got) == {"reset@1024", "parts_reversed", "groups_swapped@0", "groups_swapped@1024", "dropped@1023", "dropped@1024",
                        "repeated@1023", "repeated@1024", "ragged_first"}
    assert set(k.split("@")[0] for k in got) == set(KINDS)
    assert mc.chain([2.0 ** 53, 1.0, 1.0]) == 2.0 ** 53 and mc.chain([1.0, 1.0, 2.0 ** 53]) == 2.0 ** 53 + 2.0  # in order, each add rounded


def test_the_byte_pairs_hold_every_ordered_pair():
    for shift in (0, 1):
        yi, yf = mc.byte_pairs(shift)
        assert yf.dtype == np.uint8 and yf.size == 16 * mc.PW == yi.size
        at = (np.arange(0, yf.size, 2) + shift) % yf.size
        pairs = yf[at].astype(np.int64) * 256 + yf[(at + 1) % yf.size]
        assert np.array_equal(np.sort(pairs), np.arange(65536))
        assert (at % 4 == 3).sum() == (32768 if shift else 0)  # shifted: half the pairs straddle a dword edge


def _draws():
    got = []

    @settings(max_examples=mc.MAX_EXAMPLES, derandomize=True, database=None, deadline=None, phases=[Phase.generate],
              suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
    @given(mc.forms_case())
    def collect(case):
        got.append(case)

    collect()
    return got


def test_the_strategy_yields_every_route_built_by_construction():
    cases = _draws()
    assert len(cases) >= mc.MAX_EXAMPLES * 2 // 3
    pinned = mc.pinned_examples()
    assert [(c.route, c.variant) for c in pinned] == mc.variants()  # whatever is drawn, every route runs once
    A = 1 << 20
    for c in cases + pinned:
        size = np.dtype(c.dtype).itemsize
        assert 0 <= c.ideal_lead < 512 and c.ideal_lead % 8 == 0 and 0 <= c.fixed_lead < 512 and c.fixed_lead % size == 0, c
        ks = [k for k, _, _ in mc.launches_of(c.n, c.dtype, A + c.ideal_lead, A + c.fixed_lead)]
        want = mc.route_kernels(c)
        assert ks == want and (c.route, c.variant) in mc.variants() and c.fill in mc.FILLS, c
        assert (c.nbf == 0) == (c.route in ("ragged_only", "empty")) and c.nbf <= 40 and 0 <= c.m < mc.PW, c
    seen = Counter((c.route, c.variant) for c in cases)
    share = {r: sum(v for (q, _), v in seen.items() if q == r) / len(cases) for r in mc.ROUTES}
    print({r: round(v, 3) for r, v in share.items()}, f"{len(seen)} of {len(mc.variants())} variants drawn")
    assert len(mc.variants()) == 1 + 3 + 11 + 12 + 3 and len(seen) >= len(mc.variants()) - 4
    assert min(share.values()) >= 0.04 and min(share[r] for r in mc.ROUTES if r != "empty") >= 0.1, share
    full = [c for c in cases if c.nbf]
    assert {c.fill for c in cases} == set(mc.FILLS) and {c.nbf for c in full} >= set(mc.NBF_EDGES)
    assert {c.m for c in full} >= {0, 1, 8191} and len({c.m for c in cases} & set(mc.M_EDGES)) >= 20
    assert {c.ideal_lead % 16 for c in cases} == {0, 8} and len({c.fixed_lead % 16 for c in cases if c.route == "parts:u8"}) >= 4


def test_the_fills_are_finite_and_of_the_drawn_dtype():
    for dtype in mc.ALL_DTYPES:
        for fill in mc.FILLS:
            c = mc.Case("x", dtype, dtype, 1, 100, 0, 0, fill, 3)
            yi, yf = mc.make_data(c)
            assert yi.dtype == np.float64 and yf.dtype == np.dtype(dtype) and yi.size == yf.size == c.n, c
            s = mc.sums_ref(yi, yf)
            assert np.isfinite(s).all(), (c, s)
            if fill == "exact:0":
                assert s[0] == 0.0 and s[1] == 0.0
            if fill == "exact:-0" and np.dtype(dtype).kind == "f":
                assert np.signbit(yf.astype(np.float64) - yi).all() and not np.signbit(s[3])  # NumPy adds to +0.0
            if fill == "sat:255" and dtype not in ("int8", "bool"):
                assert s[5] == c.n
            if fill == "sat:0":
                assert s[4] == c.n
    big = mc.make_data(mc.Case("x", "float64", "float64", 40, 8191, 0, 0, "sat:max", 1))
    assert np.isfinite(mc.sums_ref(*big)).all()  # the largest drawn size still sums without overflow
