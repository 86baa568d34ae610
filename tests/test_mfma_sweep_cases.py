"""CPU: tests/mfma_sweep_cases.py is right before tests/test_gpu_mfma_sweeps.py leans on it.

* every constant (and unnamed literal) the restated launch geometry rests on reads back from the
  source file named for it: a retuned kernel fails here first, and the failure names the constant;
* the restated (k-steps per chunk, several chunks, tiles per run) of every length in
  test_gpu_long_taps.RUN_KERNEL equals that table, and the high-plane filters take the HN stated;
* every case's restated geometry gives every wave REQUIRED iterations, some waves one more, and a
  stale share within STALE_CAP; the case tables hold what they are meant to hold;
* the pooled reference is honest: oracle(pool)[idx] equals oracle(pool[idx]), both sample types and
  stages, and stale_share counts what it says on images small enough to count by hand.
"""
from __future__ import annotations

import re
from collections import Counter
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import mfma_sweep_cases as mc
from census_cases import UNREACHED
from oracle import c_oracle
from test_gpu_long_taps import RUN_KERNEL, _high_plane_form

CSRC = Path(__file__).resolve().parents[1] / "warmup-fir-filter_amd" / "csrc"


@pytest.mark.parametrize("name", list(mc.LIMITS))
def test_the_limits_are_the_sources(name):
    file, value = mc.LIMITS[name]
    m = re.search(rf"constexpr int [^;]*\b{name} = (\d+)[,;]", (CSRC / file).read_text())
    assert m and int(m.group(1)) == value, (name, file, m and m.group(1))


def test_the_unnamed_literals_are_the_sources():
    for what, (file, text) in mc.LITERALS.items():
        assert text in (CSRC / file).read_text(), (what, file)
    lim = {k: v for k, (_, v) in mc.LIMITS.items()}
    assert (mc.TILE, mc.STEP_TPS, mc.STEP_BLOCKS) == (lim["kMfTile"], lim["kMf2Tps"], lim["kMf2Blocks"])
    assert (mc.LONG_BLOCKS, mc.LONG_CHUNK) == (lim["kMlBlocks"], lim["kMlChunk"])
    assert mc.MAX_DEPTH == max(lim["kMrDepth"], lim["kMrDepth1"], lim["kMrMDepth"], 3)
    assert mc.REQUIRED == {"step": 4, "run": mc.MAX_DEPTH + 3, "long": 3}
    assert mc.STALE_CAP == 0.03 and mc.K_POOL == 127


def test_run_forms_equal_the_long_taps_table():
    for L, forms in RUN_KERNEL.items():
        if forms == "step":
            assert mc.kernel_of("u8", L) == "step" and mc.k_steps(L) == 3, L
            continue
        assert mc.kernel_of("u8", L) == "run" and mc.kernel_of("i16", L) == "long", L
        assert (mc.run_form(L, mc.U8), mc.run_form(L, mc.I32)) == forms, L
    assert set(mc.RUN_L) <= set(RUN_KERNEL)


def test_step_forms_are_the_seven_that_launch():
    """2 k-steps end at 33 taps and int16 -> int32 starts at 40: that form launches from no call
    (tests/census_cases.py says the same), so 40 taps stand in with 3 k-steps."""
    assert max(L for L in range(10, 66) if mc.k_steps(L) == 2) == 33 < mc.mfma_min_taps("i16", mc.I32) == 40
    assert "fir1d_mfma_step_kernel<short, 1, 2, *" in UNREACHED
    forms = {(d, s, mc.k_steps(L)) for d, s, L in mc.STEP_FORMS}
    assert forms == {(d, s, ks) for d in ("u8", "i16") for s in (mc.U8, mc.I32) for ks in (2, 3)} - {("i16", mc.I32, 2)}
    for d, s, L in mc.STEP_FORMS:
        assert mc.kernel_of(d, L) == "step" and L >= mc.mfma_min_taps(d, s), (d, s, L)
    modes = Counter(c.mode for c in mc.STEP_CASES if c.shape == "narrow")
    assert set(modes) == set(mc.MODES) and min(modes.values()) >= 4, modes
    full = {(c.dtype, c.stage) for c in mc.STEP_CASES if c.shape == "full"}
    assert full == {(d, s) for d in ("u8", "i16") for s in (mc.U8, mc.I32)}
    assert all(mc.k_steps(c.L) == 3 for c in mc.STEP_CASES if c.shape == "full")


def test_run_and_long_tables_hold_every_configuration():
    seen = {(c.L, c.stage, c.shape, c.mode) for c in mc.RUN_CASES if c.filt == "random" and c.shape != "flat"}
    for L in mc.RUN_L:
        for stage in (mc.U8, mc.I32):
            for shape in ("narrow", "full"):
                got = {m for (l, s, sh, m) in seen if (l, s, sh) == (L, stage, shape)}
                assert "wrap32" in got and len(got) == 2, (L, stage, shape, got)
    # what the table says differs in the loop, by L
    waves = {(L, s): mc.mr_waves_of(s, mc.run_form(L, s)[2], mc.run_form(L, s)[1], mc.run_form(L, s)[0])
             for L in mc.RUN_L for s in (mc.U8, mc.I32)}
    assert (waves[66, mc.U8], waves[66, mc.I32], waves[290, mc.U8], waves[450, mc.U8], waves[800, mc.U8]) == (4, 3, 3, 2, 1)
    assert mc.run_form(194, mc.U8)[0] == 8 and mc.run_form(450, mc.I32) == (16, False, 1)
    assert mc.run_form(720, mc.U8) == (24, False, 1) and waves[720, mc.U8] == 2  # the TRIM form: NS > 22 at 2 waves
    assert mc.run_form(720, mc.I32) == (12, True, 2) and mc.run_form(1000, mc.U8) == (6, True, 4)
    assert mc.run_form(2658, mc.U8)[:2] == (8, True) and mc.run_form(2658, mc.I32)[:2] == (8, True)
    depths = {mc.run_depth(c.stage, c.tps) for c in mc.RUN_CASES}
    assert depths == {1, 2, 3} and max(depths) == mc.MAX_DEPTH
    # the high-plane forms
    assert mc.run_form(mc.HIGH_PLANE_L, mc.U8) == (14, False, 1)
    assert set(mc.HIGH_PLANE.values()) == {0, 2, 4}
    for c in mc.RUN_CASES:
        if c.stage == mc.U8 and not mc.run_form(c.L, c.stage)[1]:  # one chunk, u8 out: the launcher picks HN from the taps
            assert _high_plane_form(np.asarray(mc.taps(c)), c.L) == c.hn, c
        if c.filt != "random":
            assert _high_plane_form(np.asarray(mc.taps(c)), c.L) == c.hn == mc.HIGH_PLANE[c.filt], c
            assert mc.MODES[c.mode][:2] == (12, 32)
    # the chunked kernel: one chunk, two, several with a short last one; both stages, shapes, modes
    assert {L: mc.long_chunks(L) for L in mc.LONG_L} == mc.LONG_CHUNKS
    assert {len(v) for v in mc.LONG_CHUNKS.values()} == {1, 2, 3} and mc.LONG_CHUNKS[1000][-1] < mc.LONG_CHUNK
    assert len(mc.LONG_CASES) == len(mc.LONG_L) * 8 == len(set(mc.LONG_CASES))
    assert {c.mode for c in mc.LONG_CASES} == {"wrap32", "acc24"}
    flat = [c for c in mc.CASES if c.shape == "flat"]
    assert [(c.kernel, c.dtype, c.stage, c.L) for c in flat] == [("step", "u8", mc.U8, 64), ("run", "u8", mc.U8, 66)]
    assert mc.geometry(flat[0]).rowlen == 9 * 8192 * 2048 // 2 + 8 and mc.geometry(flat[1]).rowlen == 13 * 4096 * 1024 // 2 + 8
    assert len({c.id for c in mc.CASES}) == len(mc.CASES)


def test_every_launch_form_is_met():
    """The three forms the launchers distinguish (no wrap possible, 32-bit wrap, fewer bits) all
    occur for each kernel, whatever the modes' names promise for a given length."""
    forms = Counter()
    for c in mc.CASES:
        frac, acc, amp = mc.MODES[c.mode]
        hq = mc.taps(c)
        assert len(hq) == c.L and -32768 <= min(hq) and max(hq) <= 32639, c  # mfma_path_ok's byte split
        if c.filt == "random":
            assert max(abs(v) for v in hq) <= amp
        forms[c.kernel, mc.form_of(c.dtype, hq, frac, acc)] += 1
        assert mc.kernel_of(c.dtype, c.L) == c.kernel, c
    assert set(forms) >= {(k, f) for k in ("step", "run") for f in ("fast", "acc32", "acc24")} | {("long", "acc32"), ("long", "acc24")}, forms


@pytest.mark.parametrize("c", mc.CASES, ids=lambda c: c.id)
def test_case_geometry_reaches_the_steady_state(c):
    g = mc.geometry(c)
    assert g.rowlen % 8 == 0 and g.ntiles == g.rows * g.tiles_per_row < 1 << 32  # mfma_path_ok
    assert g.units == mc.units_of(c.kernel, c.tps, g.rows, g.rowlen)
    assert g.waves == c.cap_waves  # the grid is capped: this is a sweep
    fewest, most = mc.iterations(SimpleNamespace(grid=(g.waves // mc.WG_WAVES, 1, 1)), g.units)
    assert fewest >= mc.REQUIRED[c.kernel] and most == fewest + 1, (fewest, most)
    last = g.units - fewest * g.waves  # the units of the last sweep: about half of one
    assert 0.4 * g.waves <= last <= 0.6 * g.waves, (last, g.waves)
    if c.kernel == "run":
        assert mc.REQUIRED["run"] >= mc.run_depth(c.stage, c.tps) + 3
    if c.tps > 1 and c.kernel != "step" and c.shape == "narrow":
        assert g.ntiles % c.tps  # the last run is partial
    if c.shape == "flat":
        assert g.rows == 1 and g.rowlen % mc.TILE == 8
        idx = np.zeros(1, np.int64)
    else:
        assert g.rowlen == mc.ROWLEN[c.shape]
        pool = mc.pool_of(c.dtype, c.shape)
        assert pool.shape == (mc.K_POOL, g.rowlen) and pool.dtype == mc.NP_DTYPE[c.dtype]
        idx = mc.canonical(pool)[mc.image_index(c, g.rows)]
    share = mc.stale_share(idx, g.tiles_per_row, c.tps, g.waves, c.kernel == "step")
    assert share <= mc.STALE_CAP, share
    name, targs, _ = mc.expected_launch(c)
    assert name == f"fir1d_mfma_{c.kernel}_kernel" and targs[0] in ("unsigned char", "short", "0", "1")


def test_pools_hold_the_extremes():
    for dtype, lo, hi in (("u8", 0, 255), ("i16", -32768, 32767)):
        pool, idx = mc.pooled(np.random.default_rng(1), mc.NP_DTYPE[dtype], 5000, 72)
        assert pool.shape == (127, 72) and idx.shape == (5000,) and set(idx) == set(range(127))
        assert (pool[0] == lo).all() and (pool[1] == hi).all()
        span = hi - lo  # uniform over the whole range: 8856 draws come within 1 % of both ends
        assert pool[4:].min() <= lo + span // 100 and pool[4:].max() >= hi - span // 100
        canon = mc.canonical(pool)
        if dtype == "u8":
            assert (pool[2] == 0).all() and (pool[3] == 128).all()
            assert canon[2] == 0 and [k for k in range(127) if canon[k] != k] == [2]
        else:
            assert (canon == np.arange(127)).all()


@pytest.mark.parametrize("dtype", ["u8", "i16"])
@pytest.mark.parametrize("stage", [mc.U8, mc.I32])
def test_pooled_reference_is_the_reference_of_the_image(dtype, stage):
    rng = np.random.default_rng(7)
    co = c_oracle()
    for rowlen, L, (frac, acc, amp) in ((72, 257, mc.MODES["wrap32"]), (1032, 64, mc.MODES["acc24"]), (2048, 20, mc.MODES["fast"])):
        pool, idx = mc.pooled(rng, mc.NP_DTYPE[dtype], 300, rowlen, K=9)
        hq = rng.integers(-amp, amp + 1, L)
        whole = co.fir1d_rows(np.ascontiguousarray(pool[idx]), hq, frac, acc, stage)
        assert np.array_equal(co.fir1d_rows(pool, hq, frac, acc, stage)[idx], whole), (rowlen, L)


def test_stale_share_counts_equal_windows():
    # one tile a row, 2 waves: units u and u + 2, u + 4, u + 6, u + 8 are compared
    idx = np.array([0, 1, 0, 2, 0, 3, 5, 1, 6, 7])
    pairs = [(u, u + 2 * d) for d in range(1, 5) for u in range(10 - 2 * d)]
    same = sum(idx[a] == idx[b] for a, b in pairs)
    assert mc.stale_share(idx, 1, 1, 2) == same / len(pairs) and same == 4
    assert mc.stale_share(np.zeros(64, int), 1, 1, 4) == 1.0  # one pool row everywhere
    assert mc.stale_share(np.arange(64), 1, 1, 4) == 0.0
    # 4 tiles a row, runs of 1: a stride of 6 tiles changes the column, one of 8 keeps it
    assert mc.stale_share(np.zeros(40, int), 4, 1, 6) < 1.0 and mc.stale_share(np.zeros(40, int), 4, 1, 8) == 1.0
    assert mc.stale_share(np.zeros(1, int), 500, 1, 8) == 0.0  # one long row: never the same column
    # runs of 2 tiles over rows of one tile: tile q of run u is row 2 u + q
    idx = np.array([0, 1, 0, 2, 3, 1, 3, 2])  # runs (0,1) (0,2) (3,1) (3,2); 1 wave: d = 1, 2, 3
    # d = 1: tile 0 of runs 0, 1 and of runs 2, 3; d = 2: tile 1 of runs 0, 2 and of runs 1, 3; d = 3: none
    assert mc.stale_share(idx, 1, 2, 1) == (2 + 2 + 0) / (6 + 4 + 2)
    # the step kernel's units stay in their row: rows of 3 tiles are steps (0, 1) and (2, -)
    assert mc.stale_share(np.zeros(8, int), 3, 2, 2, rowwise=True) == 1.0
    assert mc.stale_share(np.zeros(8, int), 3, 2, 1, rowwise=True) < 1.0
    # the partial last run's missing tile pairs with nothing
    assert mc.stale_share(np.zeros(7, int), 1, 2, 1) == 1.0


def test_unit_and_iteration_of_an_output():
    c = next(c for c in mc.STEP_CASES if c.shape == "full")
    g = mc.geometry(c)
    assert mc.unit_of(c, g, 0, 0) == (0, 0) and mc.unit_of(c, g, 0, 2047) == (1, 0) and mc.unit_of(c, g, 0, 2048) == (2, 1)
    assert mc.unit_of(c, g, 5, 4095) == (23, 11)
    c = next(c for c in mc.RUN_CASES if c.tps == 4 and c.shape == "narrow")
    g = mc.geometry(c)
    assert mc.unit_of(c, g, 9, 71) == (9, 2)
    c = next(c for c in mc.LONG_CASES if c.shape == "full")
    assert mc.unit_of(c, mc.geometry(c), 2, 1024) == (9, 9)
    # the outputs of the waves' first iterations are the prefix that ends where unit `waves` starts
    for c in mc.CASES:
        g = mc.geometry(c)
        n = mc.first_sweep_outputs(c, g, g.waves)
        assert 0 < n < g.rows * g.rowlen
        assert mc.unit_of(c, g, *divmod(n - 1, g.rowlen))[1] == g.waves - 1 and mc.unit_of(c, g, *divmod(n, g.rowlen))[1] == g.waves, c
