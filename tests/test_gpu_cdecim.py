"""GPU: the decimating complex-tap FIR (fir_cplx_decim_rows_dev of libfir_cdecim.so, through
torch_cdecim.fir1d_fixed_rows_cplx_decim_dev).

The reference for every value is tests/cdecim_cases.py's ``want``: tests/cplx_ref.py's ``want`` (two
real filters of the committed C oracle) viewed as frames and sliced ``[..., phase::D, :]``
(tests/test_cdecim_cases.py holds it against a direct Python-int loop), so every comparison is
np.array_equal, no tolerance.  Every case asserts that what the call launched (last_launch) is what
the library's route query says, and that both are what predicted_route works out from the header's
documented conditions; x and y sit inside one larger allocation each, between hostile samples and
canaries (tests/guarded.py).  No test here provokes a fault: all buffers are in bounds.

Geometry of the fast kernel (header comment of csrc_cdecim/fir1d_cplx_decim.hip).  A tile is T = 512
consecutive output frames of one row; lane u of the 256 owns outputs u and u + 256 of a tile, so a
wave's outputs are two runs of W = 64; a workgroup owns G = max(1, 16 / D) tiles and stages the
(G T - 1) D + LP input frames behind them from the 16-byte boundary below the first one.  Filters are
zero-padded to LP in {2, 4, 6, 8, 12, 16, 24, 32, 48, 64}.  So the single rows here have an out_width
one below, at and one past 1 and 257 (lane 0's two outputs), W, T, G T and 2 G T -- the widest about
16 Ki frames at every D -- taken both at the smallest width with that out_width and with D - 1 skipped
frames behind the last kept one; rows narrower than the window (1, 2 and taps - 1 frames) and rows
with phase >= width (empty).  The multi-row shapes of the fast path have rows of a multiple of 4
frames, from rows far narrower than a 64-tap window (4 and 8 frames) to rows of one workgroup's input
(G T D frames) and one 16-byte chunk more.  The generic kernels own 256 consecutive kept frames per
workgroup: rows of 1028 and 1030 frames at small D have workgroups inside one row (the wave-uniform
loop) and workgroups over a row's end (the per-lane loop).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from hypothesis import given, settings

import cdecim_cases as dc
import cplx_ref
import fir_hip
import rate_property_cases as rc
from fir_hip import cdecim, torch_cdecim, torch_cplx, torch_ops
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

DEV = torch.device("cuda:0")
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT
T, W = dc.T, dc.W


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at row {r}, kept frame {k // 2} "
                             f"({'im' if k % 2 else 're'}): {got[r, k]} != {want[r, k]}")


def _check(x, hq, D, phase=0, frac=12, acc=32, stage=I32, *, route=None, full=None, x_lead=0, y_lead=0, what=""):
    """One call on guarded buffers: predicted route == the library's route query == what was launched,
    the values equal the reference (``full``: the full-rate reference of (x, hq, frac, acc, stage),
    when the caller shares it among phases and rates), the guards hold."""
    rows, width = x.shape[0], x.shape[1] // 2
    ref = dc.sliced(full, D, phase) if full is not None else dc.want(x, hq, D, phase, frac, acc, stage)
    assert ref.shape == (rows, 2 * dc.out_width(width, D, phase)), what
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    yd, guards = guarded_output(ref.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=y_lead, device=DEV)
    pred = dc.predicted_route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, D, phase, frac, acc, stage)
    if route is not None:
        assert pred[0] == route, (what, pred)
    assert tuple(cdecim.route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, D, phase, frac, acc, stage)) == pred, what
    out = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, D, phase, frac, acc, stage, out=yd)
    assert out is yd
    assert tuple(cdecim.last_launch()) == pred, (what, cdecim.last_launch(), pred)
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), ref, what)
    guards(str(what))
    return pred


# ---- 1. fast kernel, output edges ----------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 5, 16, 33, 64])
def test_fast_kernel_output_edges(L):
    rng = np.random.default_rng(10 + L)
    hq = dc.taps(rng, L)
    bucket = min(b for b in dc.BUCKETS if b >= L)
    for D in (2, 3, 4, 8, 16):
        for i, ow in enumerate(dc.edge_out_widths(D)):
            for phase in (0, D - 1):
                width = dc.width_for(ow, D, phase, slack=(D - 1) * (i % 2))
                assert _check(dc.frames(rng, 1, width), hq, D, phase, what=(L, D, phase, width)) == (dc.FAST, bucket)
        assert dc.width_for(max(dc.edge_out_widths(D)), D, D - 1) > 15000
        for width in sorted({1, 2, max(1, L - 1)}):  # rows narrower than the window; phase >= width: empty
            x = dc.frames(rng, 1, width)
            full = cplx_ref.want(x, hq)
            for phase in (0, D - 1):
                want = (dc.FAST, bucket) if width > phase else (dc.NONE, 0)
                assert _check(x, hq, D, phase, full=full, what=(L, D, phase, width)) == want


# ---- 2. rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3, 16])
def test_fast_kernel_rows(D):
    rng = np.random.default_rng(20 + D)
    for L in (1, 2, 5, 16, 33, 64):
        hq = dc.taps(rng, L)
        for rows, width in dc.multi_row_shapes(D):
            x = dc.frames(rng, rows, width)
            full = cplx_ref.want(x, hq)
            for phase in (0, D - 1):
                want = dc.FAST if width > phase else dc.NONE
                _check(x, hq, D, phase, full=full, route=want, what=(L, D, phase, rows, width))


# ---- 3. every tap count ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_every_tap_count(D):
    """Taps 1..64 on one row of two workgroups and some and on 4 rows of 516 frames: every bucket, both
    parities of taps / 2, the centre shift; the reported bucket is the smallest that holds the taps."""
    rng = np.random.default_rng(30 + D)
    G = dc.tiles_per_group(D)
    x1, x4 = dc.frames(rng, 1, 2 * G * T * D + 37 * D + 1), dc.frames(rng, 4, 516)
    for L in range(1, 65):
        hq = dc.taps(rng, L)
        want = (dc.FAST, min(b for b in dc.BUCKETS if b >= L))
        assert _check(x1, hq, D, L % D, what=(L, D, "one row")) == want
        assert _check(x4, hq, D, (L + 1) % D, what=(L, D, "4 rows")) == want


# ---- 4. every rate and phase -----------------------------------------------------------------------
@pytest.mark.parametrize("D", range(2, 17))
def test_every_rate_and_phase(D):
    rng = np.random.default_rng(40 + D)
    hq = dc.taps(rng, 16)
    G = dc.tiles_per_group(D)
    for x in (dc.frames(rng, 1, G * T * D + 29 * D + 3), dc.frames(rng, 4, 1028)):
        full = cplx_ref.want(x, hq)
        for phase in range(D):
            assert _check(x, hq, D, phase, full=full, what=(D, phase, x.shape)) == (dc.FAST, 16)


# ---- 5. arithmetic ---------------------------------------------------------------------------------
def _runs(rng, rows, width):
    """Samples of +-32767 / -32768 in runs of random lengths."""
    ends = np.array([32767, -32768, -32767], np.int16)
    n = rows * 2 * width
    return np.repeat(ends[rng.integers(0, 3, n)], rng.integers(1, 9, n))[:n].reshape(rows, 2 * width).copy()


@pytest.mark.parametrize("acc,frac", [(32, 12), (24, 12), (32, 1), (32, 31), (24, 1), (17, 31)])
def test_wrap_and_rounding_at_the_ends_of_int16(acc, frac):
    """Taps of +-32767 over samples of +-32767 / -32768 in runs: the 32-bit sums wrap many times over
    and must agree with the oracle's single wrap to acc_bits; frac_bits 1 and 31."""
    rng = np.random.default_rng(50 + acc + frac)
    for L, D, phase in ((64, 2, 1), (33, 3, 0), (5, 16, 15), (16, 5, 2)):
        hq = np.where(rng.integers(0, 2, (L, 2)) == 0, 32767, -32767)
        for x in (_runs(rng, 1, 3000 + D), _runs(rng, 4, 1028)):
            _check(x, hq, D, phase, frac, acc, route=dc.FAST, what=(acc, frac, L, D, x.shape))


def test_real_taps_equal_the_real_decimator_and_d1_the_full_rate_filter():
    rng = np.random.default_rng(55)
    for L, D, phase, frac, acc, stage in ((9, 4, 1, 12, 32, I32), (64, 2, 0, 8, 24, I32), (70, 3, 2, 12, 32, I32),
                                          (5, 17, 4, 12, 40, I32), (7, 3, 1, 6, 32, U8)):
        x = dc.frames(rng, 4, 1028)
        hq = dc.taps(rng, L, -40, 41) if stage == U8 else dc.taps(rng, L)
        hq[:, 1] = 0
        _check(x, hq, D, phase, frac, acc, stage, what=("real taps", L, D))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, D, phase, frac, acc, stage)
        real = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq[:, 0], D, phase, frac, acc, stage, 2)
        assert got.dtype == real.dtype and torch.equal(got, real), ("real taps", L, D)
        assert np.array_equal(got.cpu().numpy(), fir_hip.fir1d_fixed_rows_decim(x, hq[:, 0], D, phase, frac, acc, stage, 2))
    for L, frac, acc, stage in ((9, 12, 32, I32), (64, 3, 24, I32), (66, 12, 32, I32), (5, 20, 40, I32), (7, 6, 32, U8)):
        x = dc.frames(rng, 3, 1030)
        hq = dc.taps(rng, L, -40, 41) if stage == U8 else dc.taps(rng, L)
        _check(x, hq, 1, 0, frac, acc, stage, what=("D = 1", L))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, 1, 0, frac, acc, stage)
        full = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage)
        assert got.dtype == full.dtype and torch.equal(got, full), ("D = 1", L)
        assert np.array_equal(got.cpu().numpy(), fir_hip.fir1d_fixed_rows_cplx(x, hq, frac, acc, stage))


# ---- 6. generic routes -----------------------------------------------------------------------------
def test_generic32_routes():
    rng = np.random.default_rng(60)
    g32 = dc.GENERIC32
    for D, phase in ((2, 1), (3, 0), (16, 7)):
        _check(dc.frames(rng, 1, 3001), dc.taps(rng, 65), D, phase, route=g32, what=("65 taps", D))
        _check(dc.frames(rng, 3, 1028), dc.taps(rng, 70), D, phase, route=g32, what=("70 taps, rows", D))
        _check(dc.frames(rng, 2, 1028), dc.taps(rng, 9, -40, 41), D, phase, 6, 32, U8, route=g32, what=("u8 stage", D))
        _check(dc.frames(rng, 1, 2500), dc.taps(rng, 16), D, phase, x_lead=4, route=g32, what=("x one frame off 16", D))
        _check(dc.frames(rng, 4, 1024), dc.taps(rng, 16), D, phase, x_lead=12, y_lead=4, route=g32, what=("x 12 off 16", D))
        _check(dc.frames(rng, 3, 1030), dc.taps(rng, 33), D, phase, route=g32, what=("rows of 4k + 2", D))
        _check(dc.frames(rng, 5, 1029), dc.taps(rng, 5), D, phase, 31, 24, route=g32, what=("odd rows", D))
        _check(dc.frames(rng, 7, 3), dc.taps(rng, 64), D, phase % 3, route=g32, what=("rows of 3 frames", D))
    for D, phase in ((17, 0), (17, 16), (40, 13), (1, 0)):
        for x in (dc.frames(rng, 1, 2 * 256 * D + 77), dc.frames(rng, 4, 1028), dc.frames(rng, 3, 1030), dc.frames(rng, 2, 5)):
            for L in (1, 16, 64, 65):
                want = g32 if x.shape[1] // 2 > phase else dc.NONE
                _check(x, dc.taps(rng, L), D, phase, route=want, what=("rate", D, phase, L, x.shape))


def test_generic64_routes():
    rng = np.random.default_rng(61)
    g64 = dc.GENERIC64
    for D, phase in ((1, 0), (2, 1), (3, 2), (16, 0), (17, 5)):
        for stage, frac in ((I32, 12), (U8, 20)):
            for x in (dc.frames(rng, 1, 1500), dc.frames(rng, 3, 1028), dc.frames(rng, 3, 258)):
                h = dc.taps(rng, 9)
                h[3, 0] = 40000
                _check(x, h, D, phase, frac, 32, stage, route=g64, what=("a tap of 40000", D, stage))
                h = dc.taps(rng, 9)
                h[2, 1] = -32768
                _check(x, h, D, phase, frac, 32, stage, route=g64, what=("a part of -32768", D, stage))
                _check(x, dc.taps(rng, 16), D, phase, 20, 40, stage, route=g64, what=("acc 40, frac 20", D, stage))
                _check(x, dc.taps(rng, 16), D, phase, 32, 32, stage, route=g64, what=("frac 32", D, stage))
                _check(x, dc.taps(rng, 5), D, phase, frac, 64, stage, route=g64, what=("acc 64", D, stage))
                _check(x, dc.taps(rng, 7), D, phase, frac, 32, stage, x_lead=2, route=g64, what=("x % 4 == 2", D, stage))
        h = dc.taps(rng, 70, -(1 << 31) + 1, 1 << 31)
        _check(dc.frames(rng, 2, 700), h, D, phase, 40, 64, route=g64, what=("int32-sized taps, no wrap", D))


def test_generic128_route():
    """needs_wide: 2^16 + 9 complex taps of +-(2^31 - 1) make sum(|hr| + |hi|) * 32768 pass 2^63, so the
    kernel sums in 128 bits.  The samples are within +-50 and a row has 150 frames, so every true sum
    stays below 150 * 2 * 2^31 * 50 < 2^46: it cannot pass 2^63, the C oracle's 64-bit sums are exact
    and ``want`` is the reference."""
    rng = np.random.default_rng(63)
    L = (1 << 16) + 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert dc.sum_can_pass_2_63(hq) and 150 * 2 * (1 << 31) * 50 < 1 << 63
    x = rng.integers(-50, 51, (2, 2 * 150), dtype=np.int16)
    for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
        full = cplx_ref.want(x, hq, frac, acc, stage)
        for phase in range(3):
            _check(x, hq, 3, phase, frac, acc, stage, full=full, route=dc.GENERIC128, what=("wide", frac, acc, phase))


# ---- 7. entry behaviour ------------------------------------------------------------------------------
def test_out_is_written_in_place_and_y_may_sit_at_any_int32_address():
    rng = np.random.default_rng(70)
    x, hq = dc.frames(rng, 4, 2052), dc.taps(rng, 24)
    full = cplx_ref.want(x, hq)
    for y_lead in (4, 8, 12, 36):
        for D, phase in ((2, 0), (3, 2), (16, 5)):
            assert _check(x, hq, D, phase, full=full, y_lead=y_lead, what=("y lead", y_lead, D)) == (dc.FAST, 24)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.full((4, 2 * dc.out_width(2052, 5, 3)), -7, dtype=torch.int32, device=DEV)
    ptr = out.data_ptr()
    got = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, torch_cdecim.CplxTaps(hq), 5, 3, out=out)
    assert got is out and out.data_ptr() == ptr
    _same(out.cpu().numpy(), dc.sliced(full, 5, 3), "out=")
    fresh = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd.reshape(2, 2, -1), hq, 5, 3)
    assert fresh.shape == (2, 2, out.shape[1]) and torch.equal(fresh.reshape(4, -1), out)
    for bad in (torch.empty((4, out.shape[1] + 2), dtype=torch.int32, device=DEV), out.to(torch.int64), out.cpu()):
        with pytest.raises(fir_hip.FirHipError):
            torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, 5, 3, out=bad)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # x's own bytes, in the shape a D = 2 call writes
        torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, 2, 0, out=xd.view(torch.int32))


def test_caller_stream():
    rng = np.random.default_rng(71)
    x, hq = dc.frames(rng, 2, 8192), dc.taps(rng, 33)
    xd = torch.from_numpy(x).to(DEV)
    yd = torch.zeros((2, 2 * dc.out_width(8192, 3, 1)), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    out = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, 3, 1, out=yd, stream=side)
    assert out is yd and tuple(cdecim.last_launch()) == (dc.FAST, 48)
    side.synchronize()  # that stream only
    _same(yd.cpu().numpy(), dc.want(x, hq, 3, 1), "side stream")


def test_fast_path_is_captured_once_and_replayed():
    """The fast path allocates nothing and reads no device table: one launch captured in a graph of
    that single launch, replayed on new input contents."""
    rng = np.random.default_rng(72)
    rows, width, D, phase = 3, 4100, 4, 3
    taps = torch_cdecim.CplxTaps(dc.taps(rng, 48))
    s = torch.cuda.Stream(device=DEV)
    x = torch.zeros((rows, 2 * width), dtype=torch.int16, device=DEV)  # static input and output
    y = torch.empty((rows, 2 * dc.out_width(width, D, phase)), dtype=torch.int32, device=DEV)
    assert dc.predicted_route(x.data_ptr(), y.data_ptr(), rows, width, taps.h, D, phase)[0] == dc.FAST
    with torch.cuda.stream(s):  # warm the entry outside the capture
        torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(x, taps, D, phase, out=y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(x, taps, D, phase, out=y)
    assert tuple(cdecim.last_launch()) == (dc.FAST, 48)
    torch.cuda.synchronize()
    for seed in (1, 2):
        xh = dc.frames(np.random.default_rng(seed), rows, width)
        x.copy_(torch.from_numpy(xh))
        y.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(y.cpu().numpy(), dc.want(xh, taps.h, D, phase), ("replay", seed))


def test_host_entry_agrees_with_the_device_entry():
    rng = np.random.default_rng(73)
    for rows, width, L, D, phase, frac, acc, stage in ((3, 2052, 33, 3, 1, 12, 32, I32), (1, 9001, 64, 16, 15, 12, 24, I32),
                                                       (2, 1030, 9, 2, 0, 6, 32, U8), (2, 600, 70, 5, 4, 20, 40, I32),
                                                       (4, 6, 5, 8, 7, 12, 32, I32)):
        x = dc.frames(rng, rows, width)
        hq = dc.taps(rng, L, -40, 41) if stage == U8 else dc.taps(rng, L)
        host = fir_hip.fir1d_fixed_rows_cplx_decim(x, hq, D, phase, frac, acc, stage)
        launched = tuple(cdecim.last_launch())
        # the host form's device buffers come from hipMalloc: 16-byte aligned
        assert launched == dc.predicted_route(0, 0, rows, width, hq, D, phase, frac, acc, stage), (rows, width, L, D)
        dev = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(torch.from_numpy(x).to(DEV), hq, D, phase, frac, acc, stage)
        assert np.array_equal(host, dev.cpu().numpy())
        _same(host, dc.want(x, hq, D, phase, frac, acc, stage), ("host", rows, width, L, D))
    out = np.empty((3, 5, 2 * dc.out_width(40, 3, 2)), np.int32)
    x = dc.frames(rng, 15, 40).reshape(3, 5, 80)
    hq = dc.taps(rng, 5)
    assert cdecim.fir1d_fixed_rows_cplx_decim(x, hq, 3, 2, out=out) is out
    _same(out.reshape(15, -1), dc.want(x.reshape(15, 80), hq, 3, 2), "host out=")


# ---- 8. random cases ---------------------------------------------------------------------------------
@settings(max_examples=60, **SETTINGS)
@given(dc.property_case())
def test_random_cases_vs_oracle(case):
    why, c = case
    x = rc.samples(c)
    hq = np.asarray(c.hq, dtype=np.int64)
    route, _ = _check(x, hq, c.decim, c.phase, c.frac, c.acc, c.stage, x_lead=c.x_lead, y_lead=c.y_lead, what=(why, c))
    if dc.out_width(c.width, c.decim, c.phase):
        assert (route == dc.FAST) == (why == ""), (why, c, route)
