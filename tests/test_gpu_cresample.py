"""GPU: the rational resampling complex-tap FIR (fir_cplx_resample_rows_dev of libfir_cresample.so,
through torch_cresample.fir1d_fixed_rows_cplx_resample_dev).

The reference for every value is tests/cresample_cases.py's ``want``: tests/cinterp_cases.py's ``want``
(two real filters of the committed C oracle on the zero-stuffed signal) sliced ``[:, phase::D]``
(tests/test_cresample_cases.py holds it against the header's polyphase formula in Python ints), so
every comparison is np.array_equal, no tolerance.  Every case asserts that what the call launched
(last_launch) is what the library's route query says, and that both are what predicted_route works out
from the header's documented conditions; x and y sit inside one larger allocation each, between
hostile samples and canaries (tests/guarded.py).  No test here provokes a fault: all buffers are in
bounds.

Geometry of the fast kernel (header comment of csrc_cresample/fir1d_cplx_resample.hip).  One period is
D input frames and U output frames.  A workgroup owns P periods of one row (512 at D = 2 or 3, else
256) and works through them as tiles of T periods (P, or 256 from U = 5 on); a tile is computed in
passes of 256 periods, lane u owning period u of each pass, so a lane's run is U output frames and a
wave's run 64 U.  Each tile's T U output frames go through an LDS stage and out as 16-byte vectors, with
the partial vectors at both ends written dword by dword.  Each phase's sub-filter is zero-padded to a
bucket in {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32}.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from hypothesis import given, settings

import cresample_cases as cc
import fir_hip
import rate_property_cases as rc
from fir_hip import cresample, torch_cdecim, torch_cinterp, torch_cplx, torch_cresample, torch_resample
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

DEV = torch.device("cuda:0")
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at row {r}, output frame {k // 2} "
                             f"({'im' if k % 2 else 're'}): {got[r, k]} != {want[r, k]}")


def _check(x, hq, U, D, phase=0, frac=12, acc=32, stage=I32, *, route=None, ref=None, x_lead=0, y_lead=0, what=""):
    """One call on guarded buffers: predicted route == the library's route query == what was launched,
    the values equal the reference (``ref``: when the caller has it already), the guards hold."""
    rows, width = x.shape[0], x.shape[1] // 2
    if ref is None:
        ref = cc.want(x, hq, U, D, phase, frac, acc, stage)
    assert ref.shape == (rows, 2 * cc.out_width(width, U, D, phase)), what
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    yd, guards = guarded_output(ref.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=y_lead, device=DEV)
    pred = cc.predicted_route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, U, D, phase, frac, acc, stage)
    if route is not None:
        assert pred[0] == route, (what, pred)
    assert tuple(cresample.route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, U, D, phase, frac, acc, stage)) == pred, what
    out = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, D, phase, frac, acc, stage, out=yd)
    assert out is yd
    assert tuple(cresample.last_launch()) == pred, (what, cresample.last_launch(), pred)
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), ref, what)
    guards(str(what))
    return pred


_EDGE_RATES = [(3, 2), (2, 3), (4, 6), (16, 15), (15, 16), (2, 16), (16, 2), (16, 16)]


# ---- 1. fast kernel, output edges, single row ----------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, -1])
@pytest.mark.parametrize("U,D", _EDGE_RATES)
def test_fast_kernel_output_edges(U, D, which):
    """The row's last output frame one below, at and one past 1 frame, a lane's run, a wave's run, a
    pass, a tile, a workgroup and two workgroups; rows narrower than the window."""
    phase = (0, 1, D - 1)[which]
    rng = np.random.default_rng(1000 * U + 10 * D + phase)
    for L in (1, 2, 5, 16, 33, 64, 128):
        if L > cc.fast_max_taps(U):  # 128 (and 64 taps at U = 2 is the last) only where the header keeps it fast
            continue
        hq = cc.taps(rng, L)
        want = (cc.FAST, cc.bucket(L, U, D, phase))
        narrow = {1, 2, max(1, -(-L // U) - 1)}  # rows narrower than the window
        for width in sorted(set(cc.edge_widths(U, D)) | narrow):
            if width * U <= phase:
                continue
            x = cc.frames(rng, 1, width)
            assert _check(x, hq, U, D, phase, what=(L, U, D, phase, width)) == want


def test_nothing_is_launched_when_the_stuffed_row_ends_before_the_phase():
    """mid_width <= phase: out_width 0, route NONE, nothing launched and y untouched."""
    rng = np.random.default_rng(5)
    hq = cc.taps(rng, 9)
    for rows, width, U, D, phase in ((1, 1, 2, 16, 5), (3, 4, 3, 16, 12), (2, 1, 16, 17, 16), (1, 2, 2, 5, 4)):
        xd = torch.from_numpy(cc.frames(rng, rows, width)).to(DEV)
        _check(cc.frames(rng, 1, 64), hq, 3, 2)  # so that last_launch holds a launch
        guard = torch.full((64,), -7, dtype=torch.int32, device=DEV)
        out = guard[32:32].view(rows, 0) if rows == 1 else torch.empty((rows, 0), dtype=torch.int32, device=DEV)
        assert cc.predicted_route(xd.data_ptr(), 0, rows, width, hq, U, D, phase) == (cc.NONE, 0)
        assert tuple(cresample.route(xd.data_ptr(), 0, rows, width, hq, U, D, phase)) == (cc.NONE, 0)
        got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, D, phase, out=out)
        assert got.shape == (rows, 0) and tuple(cresample.last_launch()) == (cc.NONE, 0)
        torch.cuda.synchronize()
        assert bool((guard == -7).all())


# ---- 2. rows of a multiple of 4 frames -------------------------------------------------------------
@pytest.mark.parametrize("U,D,phase", [(3, 2, 1), (2, 3, 0), (16, 15, 14), (5, 16, 7), (16, 16, 15)])
def test_fast_kernel_rows(U, D, phase):
    """No frame of a neighbouring row leaks in at either end: rows far narrower than a window, 300
    rows of 4 frames, rows of one workgroup's frames and 4 more, a last tile partly empty."""
    rng = np.random.default_rng(20 + 100 * U + D)
    for L in (1, 2, 5, 16, 33, 64):
        hq = cc.taps(rng, L)
        for rows, width in cc.multi_row_shapes(U, D):
            _check(cc.frames(rng, rows, width), hq, U, D, phase, route=cc.FAST, what=(L, U, D, rows, width))


# ---- 3. every tap count ----------------------------------------------------------------------------
@pytest.mark.parametrize("U,D", [(3, 2), (2, 3)])
def test_every_tap_count(U, D):
    """Taps 1 .. the fast limit on one row of two workgroups and a bit more and on 4 rows of 516
    frames: every bucket, every empty phase, both parities of taps / 2, the centre shift; the reported
    bucket is the one the header's rule gives."""
    rng = np.random.default_rng(30 + U)
    x1, x4 = cc.frames(rng, 1, 2 * cc.periods(D) * D + 37), cc.frames(rng, 4, 516)
    seen = set()
    for L in range(1, cc.fast_max_taps(U) + 1):
        hq = cc.taps(rng, L)
        phase = L % D
        want = (cc.FAST, cc.bucket(L, U, D, phase))
        seen.add(want[1])
        assert _check(x1, hq, U, D, phase, what=(L, U, D, "one row")) == want
        assert _check(x4, hq, U, D, phase, what=(L, U, D, "4 rows")) == want
    assert seen == set(cc.BUCKETS), seen


# ---- 4. every rate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("U", range(2, 17))
def test_every_rate(U):
    """Every D in {2, 3, 5, 8, 16} with 16 taps and with U - 1 taps (some phases empty) on both shapes
    of the tap-count test; every phase for D <= 3, a phase that moves with U beyond."""
    rng = np.random.default_rng(40 + U)
    for D in (2, 3, 5, 8, 16):
        x1, x4 = cc.frames(rng, 1, 2 * cc.periods(D) * D + 29), cc.frames(rng, 4, 516)
        for phase in (range(D) if D <= 3 else [(3 * U + 1) % D]):
            for L in (16, U - 1):
                hq = cc.taps(rng, L)
                for x in (x1, x4):
                    assert _check(x, hq, U, D, phase, what=(U, D, phase, L, x.shape)) == (cc.FAST, cc.bucket(L, U, D, phase))


# ---- 5. arithmetic ---------------------------------------------------------------------------------
def _runs(rng, rows, width):
    """Samples of +-32767 / -32768 in runs of random lengths."""
    ends = np.array([32767, -32768, -32767], np.int16)
    n = rows * 2 * width
    return np.repeat(ends[rng.integers(0, 3, n)], rng.integers(1, 9, n))[:n].reshape(rows, 2 * width).copy()


@pytest.mark.parametrize("acc", [8, 16, 31, 32])
@pytest.mark.parametrize("frac", [1, 12, 31])
def test_wrap_and_rounding_at_the_ends_of_int16(acc, frac):
    """Taps of +-32767 over samples of +-32767 / -32768 in runs: the 32-bit sums wrap many times over
    and must agree with the oracle's single wrap to acc_bits."""
    rng = np.random.default_rng(50 + acc + frac)
    for L, U, D, phase in ((64, 2, 3, 1), (33, 3, 2, 0), (128, 16, 15, 7), (16, 5, 8, 3)):
        hq = np.where(rng.integers(0, 2, (L, 2)) == 0, 32767, -32767)
        for x in (_runs(rng, 1, 1500 + U), _runs(rng, 4, 260)):
            _check(x, hq, U, D, phase, frac, acc, route=cc.FAST, what=(acc, frac, L, U, D, x.shape))


@pytest.mark.parametrize("acc", [33, 48, 64])
def test_generic64_sums(acc):
    rng = np.random.default_rng(60 + acc)
    for U, D, phase in ((1, 1, 0), (3, 2, 1), (2, 3, 2), (16, 17, 5), (17, 4, 0), (1, 5, 3), (4, 1, 0)):
        for stage, frac in ((I32, 12), (I32, 40), (U8, 20)):
            for x in (cc.frames(rng, 1, 700), cc.frames(rng, 3, 260), cc.frames(rng, 3, 5)):
                _check(x, cc.taps(rng, 16), U, D, phase, frac, acc, stage, route=cc.GENERIC64, what=(acc, U, D, frac, stage, x.shape))
        h = cc.taps(rng, 70, -(1 << 31) + 1, 1 << 31)
        _check(cc.frames(rng, 2, 300), h, U, D, phase, 40, acc, route=cc.GENERIC64, what=("int32-sized taps", acc, U, D))


def test_generic128_route():
    """needs_wide: 2^16 + 9 complex taps of +-(2^31 - 1) make sum(|hr| + |hi|) * 32768 pass 2^63, so the
    kernel sums in 128 bits.  The reference is want_loop (unbounded Python ints), the only one that
    holds whatever a sum reaches; its loop is as long as the row, whatever the tap count."""
    rng = np.random.default_rng(63)
    L = (1 << 16) + 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert cc.sum_can_pass_2_63(hq)
    x = _runs(rng, 2, 40)
    for U, D, phase, frac, acc, stage in ((3, 2, 1, 30, 64, I32), (2, 3, 0, 45, 80, U8), (1, 1, 0, 30, 64, I32), (17, 5, 4, 36, 64, I32)):
        ref = cc.want_loop(x, hq, U, D, phase, frac, acc, stage)
        _check(x, hq, U, D, phase, frac, acc, stage, ref=ref, route=cc.GENERIC128, what=("wide", U, D, frac, acc))


def test_a_tap_part_past_int16_leaves_the_fast_path():
    rng = np.random.default_rng(61)
    for U, D, phase in ((3, 2, 1), (2, 3, 0), (16, 16, 9)):
        for x in (cc.frames(rng, 1, 1500), cc.frames(rng, 3, 260)):
            for poke, at in ((32768, 0), (-32768, 1), (-32768, 0), (32768, 1), (40000, 0)):
                h = cc.taps(rng, 9)
                h[3, at] = poke
                _check(x, h, U, D, phase, route=cc.GENERIC64, what=("a part of", poke, U, D))
            h = cc.taps(rng, 9)
            h[3] = (32767, -32767)
            _check(x, h, U, D, phase, route=cc.FAST, what=("parts of +-32767", U, D))


def test_each_generic32_reason_on_its_own():
    rng = np.random.default_rng(62)
    g32 = cc.GENERIC32
    for U, D, phase in ((3, 2, 1), (2, 3, 2), (16, 15, 0)):
        L = cc.fast_max_taps(U) + 1
        _check(cc.frames(rng, 1, 1501), cc.taps(rng, L), U, D, phase, route=g32, what=("one tap too many", L, U, D))
        _check(cc.frames(rng, 3, 260), cc.taps(rng, 140), U, D, phase, route=g32, what=("140 taps, rows", U, D))
        _check(cc.frames(rng, 2, 260), cc.taps(rng, 9, -40, 41), U, D, phase, 6, 32, U8, route=g32, what=("u8 stage", U, D))
        _check(cc.frames(rng, 7, 3), cc.taps(rng, 64), U, D, phase, route=g32, what=("rows of 3 frames", U, D))
        _check(cc.frames(rng, 5, 257), cc.taps(rng, 5), U, D, phase, 31, 24, route=g32, what=("odd rows", U, D))
        _check(cc.frames(rng, 1, 1501), cc.taps(rng, 24), U, D, phase, x_lead=4, route=g32, what=("x off 16", U, D))
    for U, D, phase in ((1, 2, 1), (2, 1, 0), (1, 1, 0), (17, 3, 2), (3, 17, 14), (40, 33, 5)):  # 5 frames at U = 3 still reach phase 14
        for x in (cc.frames(rng, 1, 777), cc.frames(rng, 4, 260), cc.frames(rng, 3, 258), cc.frames(rng, 2, 5)):
            for L in (1, 16, 64, 129):
                _check(x, cc.taps(rng, L), U, D, phase, route=g32, what=("rate", U, D, L, x.shape))
    _check(cc.frames(rng, 2, 260), cc.taps(rng, 16), 3, 2, 0, 32, 32, route=cc.GENERIC64, what="frac 32")
    _check(cc.frames(rng, 2, 260), cc.taps(rng, 7), 3, 2, 0, x_lead=2, route=cc.GENERIC64, what="x % 4 == 2")


# ---- 6. identities on the device -------------------------------------------------------------------
_BITS = ((12, 32, I32), (3, 24, I32), (20, 40, I32), (6, 32, U8))


def test_decim_1_is_the_interpolator():
    rng = np.random.default_rng(64)
    for (frac, acc, stage), (L, U) in zip(_BITS, ((33, 3), (64, 2), (5, 16), (7, 4))):
        x = cc.frames(rng, 3, 1028)
        hq = cc.taps(rng, L, -40, 41) if stage == U8 else cc.taps(rng, L)
        _check(x, hq, U, 1, 0, frac, acc, stage, what=("D = 1", L, U))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, 1, 0, frac, acc, stage)
        ref = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, U, frac, acc, stage)
        assert got.dtype == ref.dtype and torch.equal(got, ref), ("D = 1", L, U)


def test_up_1_is_the_decimator():
    rng = np.random.default_rng(65)
    for (frac, acc, stage), (L, D, phase) in zip(_BITS, ((33, 3, 2), (64, 2, 0), (5, 16, 9), (7, 4, 1))):
        x = cc.frames(rng, 3, 1028)
        hq = cc.taps(rng, L, -40, 41) if stage == U8 else cc.taps(rng, L)
        _check(x, hq, 1, D, phase, frac, acc, stage, what=("U = 1", L, D))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, 1, D, phase, frac, acc, stage)
        ref = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, hq, D, phase, frac, acc, stage)
        assert got.dtype == ref.dtype and torch.equal(got, ref), ("U = 1", L, D)


def test_up_1_decim_1_is_the_full_rate_filter():
    rng = np.random.default_rng(66)
    for (frac, acc, stage), L in zip(_BITS, (9, 64, 66, 7)):
        x = cc.frames(rng, 3, 1030)
        hq = cc.taps(rng, L, -40, 41) if stage == U8 else cc.taps(rng, L)
        _check(x, hq, 1, 1, 0, frac, acc, stage, what=("U = D = 1", L))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, 1, 1, 0, frac, acc, stage)
        full = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage)
        assert got.dtype == full.dtype and torch.equal(got, full), ("U = D = 1", L)


def test_real_taps_equal_the_real_resampler():
    rng = np.random.default_rng(67)
    for L, U, D, phase, frac, acc, stage in ((9, 4, 3, 1, 12, 32, I32), (64, 2, 3, 0, 8, 24, I32), (128, 16, 15, 14, 12, 32, I32),
                                             (140, 3, 2, 1, 12, 32, I32), (5, 17, 4, 2, 12, 40, I32), (7, 3, 5, 4, 6, 32, U8)):
        x = cc.frames(rng, 4, 516)
        hq = cc.taps(rng, L, -40, 41) if stage == U8 else cc.taps(rng, L)
        hq[:, 1] = 0
        _check(x, hq, U, D, phase, frac, acc, stage, what=("real taps", L, U, D))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, D, phase, frac, acc, stage)
        real = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq[:, 0], U, D, phase, frac, acc, stage, 2)
        assert got.dtype == real.dtype and torch.equal(got, real), ("real taps", L, U, D)


def test_one_call_equals_the_two_call_form():
    """The interpolator into a width * U intermediate, then [..., phase::D, :]: what a caller did before."""
    rng = np.random.default_rng(68)
    for L, U, D, phase in ((72, 3, 2, 1), (64, 2, 3, 2), (64, 4, 6, 5), (128, 8, 5, 0), (128, 16, 15, 14), (40, 17, 3, 1)):
        for x in (cc.frames(rng, 1, 2 * cc.periods(min(D, 16)) * D + 21), cc.frames(rng, 4, 516)):
            hq = cc.taps(rng, L)
            xd = torch.from_numpy(x).to(DEV)
            got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, D, phase)
            assert (cresample.last_launch().route == cc.FAST) == (U <= 16)
            mid = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, U)
            two = mid.view(x.shape[0], -1, 2)[:, phase::D, :].contiguous().view(x.shape[0], -1)
            assert torch.equal(got, two), (L, U, D, phase, x.shape)


# ---- 7. addressing and capture -----------------------------------------------------------------------
def test_y_at_every_int32_offset_and_x_at_16_byte_offsets():
    rng = np.random.default_rng(70)
    hq = cc.taps(rng, 24)
    for U, D, phase in ((3, 2, 1), (2, 3, 0), (16, 15, 3)):
        x, x1 = cc.frames(rng, 4, 516), cc.frames(rng, 1, 2 * cc.periods(D) * D + 37)
        ref, ref1 = cc.want(x, hq, U, D, phase), cc.want(x1, hq, U, D, phase)
        want = (cc.FAST, cc.bucket(24, U, D, phase))
        for y_lead in (0, 4, 8, 12, 36):
            for x_lead in (0, 16, 48):
                assert _check(x, hq, U, D, phase, ref=ref, x_lead=x_lead, y_lead=y_lead, what=("rows", U, D, x_lead, y_lead)) == want
            assert _check(x1, hq, U, D, phase, ref=ref1, x_lead=32, y_lead=y_lead, what=("one row", U, D, y_lead)) == want
        for x_lead in (4, 8, 12):  # x off 16 bytes: the generic kernel, the same values
            _check(x, hq, U, D, phase, ref=ref, x_lead=x_lead, y_lead=x_lead, route=cc.GENERIC32, what=("x off 16", U, D, x_lead))
            _check(x1, hq, U, D, phase, ref=ref1, x_lead=x_lead, route=cc.GENERIC32, what=("one row, x off 16", U, D, x_lead))
        for width in (513, 514, 515):  # rows that do not start as x does
            _check(cc.frames(rng, 3, width), hq, U, D, phase, route=cc.GENERIC32, what=("rows of", width, U, D))


def test_out_is_written_in_place():
    rng = np.random.default_rng(71)
    x, hq = cc.frames(rng, 4, 516), cc.taps(rng, 24)
    U, D, phase = 5, 3, 2
    ref = cc.want(x, hq, U, D, phase)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.full(ref.shape, -7, dtype=torch.int32, device=DEV)
    ptr = out.data_ptr()
    got = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, torch_cresample.CplxTaps(hq), U, D, phase, out=out)
    assert got is out and out.data_ptr() == ptr
    _same(out.cpu().numpy(), ref, "out=")
    fresh = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd.reshape(2, 2, -1), hq, U, D, phase)
    assert fresh.shape == (2, 2, out.shape[1]) and torch.equal(fresh.reshape(4, -1), out)
    for bad in (torch.empty((4, out.shape[1] + 2), dtype=torch.int32, device=DEV), out.to(torch.int64), out.cpu()):
        with pytest.raises(fir_hip.FirHipError):
            torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, U, D, phase, out=bad)
    big = torch.zeros(4096, dtype=torch.int16, device=DEV)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # 64 frames of x inside the bytes a 3 / 2 call writes
        torch_cresample.fir1d_fixed_rows_cplx_resample_dev(big[:128].view(1, 128), hq, 3, 2, out=big.view(torch.int32)[8:200].view(1, 192))
    for bad, text in (((0, 2, 0), "up must be >= 1"), ((2, 0, 0), "decim must be >= 1"), ((2, 3, 3), "phase must be in"),
                      ((2, 3, -1), "phase must be in")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, *bad)


def test_caller_stream():
    rng = np.random.default_rng(72)
    x, hq = cc.frames(rng, 2, 4096), cc.taps(rng, 33)
    xd = torch.from_numpy(x).to(DEV)
    ref = cc.want(x, hq, 3, 2, 1)
    yd = torch.zeros(ref.shape, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    out = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, hq, 3, 2, 1, out=yd, stream=side)
    assert out is yd and tuple(cresample.last_launch()) == (cc.FAST, cc.bucket(33, 3, 2, 1))
    side.synchronize()  # that stream only
    _same(yd.cpu().numpy(), ref, "side stream")


def _capture_and_replay(rows, width, U, D, phase, taps, want_route):
    s = torch.cuda.Stream(device=DEV)
    x = torch.zeros((rows, 2 * width), dtype=torch.int16, device=DEV)  # static input and output
    y = torch.empty((rows, 2 * cc.out_width(width, U, D, phase)), dtype=torch.int32, device=DEV)
    assert cc.predicted_route(x.data_ptr(), y.data_ptr(), rows, width, taps.h, U, D, phase) == want_route
    with torch.cuda.stream(s):  # warm the entry outside the capture (a generic call's table is uploaded here)
        torch_cresample.fir1d_fixed_rows_cplx_resample_dev(x, taps, U, D, phase, out=y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        torch_cresample.fir1d_fixed_rows_cplx_resample_dev(x, taps, U, D, phase, out=y)
    assert tuple(cresample.last_launch()) == want_route
    torch.cuda.synchronize()
    for seed in (1, 2):
        xh = cc.frames(np.random.default_rng(seed), rows, width)
        x.copy_(torch.from_numpy(xh))
        y.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(y.cpu().numpy(), cc.want(xh, taps.h, U, D, phase), ("replay", seed, want_route))


def test_fast_path_is_captured_once_and_replayed():
    """The fast path allocates nothing and reads no device table: one launch captured on a side stream
    in a graph of that single kernel, replayed twice on input changed in place."""
    rng = np.random.default_rng(73)
    _capture_and_replay(3, 2052, 4, 3, 2, torch_cresample.CplxTaps(cc.taps(rng, 48)), (cc.FAST, cc.bucket(48, 4, 3, 2)))


def test_warmed_up_generic_call_is_captured_too():
    rng = np.random.default_rng(74)
    _capture_and_replay(3, 1030, 4, 3, 2, torch_cresample.CplxTaps(cc.taps(rng, 48)), (cc.GENERIC32, 0))


def test_host_entry_agrees_with_the_device_entry():
    rng = np.random.default_rng(75)
    for rows, width, L, U, D, phase, frac, acc, stage in (
            (3, 516, 33, 3, 2, 1, 12, 32, I32), (1, 2101, 128, 16, 15, 4, 12, 24, I32), (2, 258, 9, 2, 3, 0, 6, 32, U8),
            (2, 300, 70, 5, 4, 3, 20, 40, I32), (4, 6, 5, 8, 7, 6, 12, 32, I32), (2, 260, 9, 1, 1, 0, 12, 32, I32)):
        x = cc.frames(rng, rows, width)
        hq = cc.taps(rng, L, -40, 41) if stage == U8 else cc.taps(rng, L)
        host = fir_hip.fir1d_fixed_rows_cplx_resample(x, hq, U, D, phase, frac, acc, stage)
        launched = tuple(cresample.last_launch())
        # the host form's device buffers come from hipMalloc: 16-byte aligned
        assert launched == cc.predicted_route(0, 0, rows, width, hq, U, D, phase, frac, acc, stage), (rows, width, L, U, D)
        dev = torch_cresample.fir1d_fixed_rows_cplx_resample_dev(torch.from_numpy(x).to(DEV), hq, U, D, phase, frac, acc, stage)
        assert np.array_equal(host, dev.cpu().numpy())
        _same(host, cc.want(x, hq, U, D, phase, frac, acc, stage), ("host", rows, width, L, U, D))
    x = cc.frames(rng, 15, 40).reshape(3, 5, 80)
    hq = cc.taps(rng, 5)
    out = np.empty((3, 5, 2 * cc.out_width(40, 3, 2, 1)), np.int32)
    assert cresample.fir1d_fixed_rows_cplx_resample(x, hq, 3, 2, 1, out=out) is out
    _same(out.reshape(15, -1), cc.want(x.reshape(15, 80), hq, 3, 2, 1), "host out=")


# ---- 8. random cases ---------------------------------------------------------------------------------
@settings(max_examples=60, **SETTINGS)
@given(cc.property_case())
def test_random_cases_vs_oracle(case):
    why, c = case
    x = rc.samples(c)
    hq = np.asarray(c.hq, dtype=np.int64)
    route, _ = _check(x, hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage, x_lead=c.x_lead, y_lead=c.y_lead, what=(why, c))
    assert (route == cc.FAST) == (why == ""), (why, c, route)
