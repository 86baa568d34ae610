"""GPU: the interpolating complex-tap FIR (fir_cplx_interp_rows_dev of libfir_cinterp.so, through
torch_cinterp.fir1d_fixed_rows_cplx_interp_dev).

The reference for every value is tests/cinterp_cases.py's ``want``: tests/cplx_ref.py's ``want`` (two
real filters of the committed C oracle) on the zero-stuffed signal (tests/test_cinterp_cases.py holds
it against the header's polyphase formula in Python ints), so every comparison is np.array_equal, no
tolerance.  Every case asserts that what the call launched (last_launch) is what the library's route
query says, and that both are what predicted_route works out from the header's documented
conditions; x and y sit inside one larger allocation each, between hostile samples and canaries
(tests/guarded.py).  No test here provokes a fault: all buffers are in bounds.

Geometry of the fast kernel (header comment of csrc_cinterp/fir1d_cplx_interp.hip).  A workgroup owns
F = 2048 consecutive input frames of one row and works through them as tiles of T input frames
(T = 1024, 512, 512, 256 at U = 2, 3, 4, 5 and up); a tile is computed in passes of 256 frames, lane u
owning input frame u of each pass, so a lane's run is one frame and a wave's run W = 64.  Each tile's
T * U output frames go through an LDS stage and out as 16-byte vectors, with the partial vectors at
both ends written dword by dword.  The per-phase window is zero-padded to a bucket in {1, 2, 3, 4, 6,
8, 10, 12, 16, 20, 24, 28, 33}.  So the single rows here have a width one below, at and one past 1, W,
256, T, F and 2 F, and rows narrower than the window; the multi-row shapes have rows of a multiple of 4
frames, from rows far narrower than a window (4 and 8 frames) to rows of F and F + 4 frames.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from hypothesis import given, settings

import cinterp_cases as ic
import fir_hip
import rate_property_cases as rc
from fir_hip import cinterp, torch_cdecim, torch_cinterp, torch_cplx, torch_interp
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

DEV = torch.device("cuda:0")
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT
F, W = ic.F, ic.W


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at row {r}, output frame {k // 2} "
                             f"({'im' if k % 2 else 're'}): {got[r, k]} != {want[r, k]}")


def _check(x, hq, U, frac=12, acc=32, stage=I32, *, route=None, ref=None, x_lead=0, y_lead=0, what=""):
    """One call on guarded buffers: predicted route == the library's route query == what was launched,
    the values equal the reference (``ref``: when the caller has it already), the guards hold."""
    rows, width = x.shape[0], x.shape[1] // 2
    if ref is None:
        ref = ic.want(x, hq, U, frac, acc, stage)
    assert ref.shape == (rows, 2 * width * U), what
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    yd, guards = guarded_output(ref.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=y_lead, device=DEV)
    pred = ic.predicted_route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, U, frac, acc, stage)
    if route is not None:
        assert pred[0] == route, (what, pred)
    assert tuple(cinterp.route(xd.data_ptr(), yd.data_ptr(), rows, width, hq, U, frac, acc, stage)) == pred, what
    out = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, U, frac, acc, stage, out=yd)
    assert out is yd
    assert tuple(cinterp.last_launch()) == pred, (what, cinterp.last_launch(), pred)
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), ref, what)
    guards(str(what))
    return pred


# ---- 1. fast kernel, output edges, single row ----------------------------------------------------
@pytest.mark.parametrize("U", [2, 3, 4, 8, 16])
def test_fast_kernel_output_edges(U):
    rng = np.random.default_rng(10 + U)
    for L in (1, 2, 5, 16, 33, 64, 128):
        if L > ic.fast_max_taps(U):  # 128 (and 64 taps at U = 2 is the last) only where the header keeps it fast
            continue
        hq = ic.taps(rng, L)
        want = (ic.FAST, ic.bucket(L, U))
        narrow = {1, 2, max(1, -(-L // U) - 1)}  # rows narrower than the window
        for width in sorted(set(ic.edge_widths(U)) | narrow):
            assert _check(ic.frames(rng, 1, width), hq, U, what=(L, U, width)) == want


# ---- 2. rows of a multiple of 4 frames -------------------------------------------------------------
@pytest.mark.parametrize("U", [2, 3, 16])
def test_fast_kernel_rows(U):
    """No frame of a neighbouring row leaks in at either end: rows far narrower than a window, 300
    rows of 4 frames, rows of F and F + 4, a last workgroup and a last tile partly empty."""
    rng = np.random.default_rng(20 + U)
    for L in (1, 2, 5, 16, 33, 64):
        hq = ic.taps(rng, L)
        for rows, width in ic.multi_row_shapes(U):
            _check(ic.frames(rng, rows, width), hq, U, route=ic.FAST, what=(L, U, rows, width))


# ---- 3. every tap count ----------------------------------------------------------------------------
@pytest.mark.parametrize("U", [2, 3])
def test_every_tap_count(U):
    """Taps 1 .. the fast limit on one row of two workgroups and a bit more and on 4 rows of 516
    frames: every bucket, every empty phase, both parities of taps / 2, the centre shift; the reported
    bucket is the one the header's rule gives."""
    rng = np.random.default_rng(30 + U)
    x1, x4 = ic.frames(rng, 1, 2 * F + 37), ic.frames(rng, 4, 516)
    seen = set()
    for L in range(1, ic.fast_max_taps(U) + 1):
        hq = ic.taps(rng, L)
        want = (ic.FAST, ic.bucket(L, U))
        seen.add(want[1])
        assert _check(x1, hq, U, what=(L, U, "one row")) == want
        assert _check(x4, hq, U, what=(L, U, "4 rows")) == want
    assert seen == set(ic.BUCKETS), seen


# ---- 4. every rate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("U", range(2, 17))
def test_every_rate(U):
    """16 taps, and U - 1 taps (some phases empty), on both shapes of the tap-count test."""
    rng = np.random.default_rng(40 + U)
    for L in (16, U - 1):
        hq = ic.taps(rng, L)
        for x in (ic.frames(rng, 1, 2 * F + 29), ic.frames(rng, 4, 516)):
            assert _check(x, hq, U, what=(U, L, x.shape)) == (ic.FAST, ic.bucket(L, U))


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
    for L, U in ((64, 2), (33, 3), (128, 16), (16, 5)):
        hq = np.where(rng.integers(0, 2, (L, 2)) == 0, 32767, -32767)
        for x in (_runs(rng, 1, 1500 + U), _runs(rng, 4, 260)):
            _check(x, hq, U, frac, acc, route=ic.FAST, what=(acc, frac, L, U, x.shape))


@pytest.mark.parametrize("acc", [33, 48, 63, 64])
def test_generic64_sums(acc):
    rng = np.random.default_rng(60 + acc)
    for U in (1, 2, 3, 16, 17):
        for stage, frac in ((I32, 12), (I32, 40), (U8, 20)):
            for x in (ic.frames(rng, 1, 700), ic.frames(rng, 3, 260), ic.frames(rng, 3, 5)):
                _check(x, ic.taps(rng, 16), U, frac, acc, stage, route=ic.GENERIC64, what=(acc, U, frac, stage, x.shape))
        h = ic.taps(rng, 70, -(1 << 31) + 1, 1 << 31)
        _check(ic.frames(rng, 2, 300), h, U, 40, acc, route=ic.GENERIC64, what=("int32-sized taps", acc, U))


def test_a_tap_part_past_int16_leaves_the_fast_path():
    rng = np.random.default_rng(61)
    for U in (1, 2, 3, 16, 17):
        for stage, frac in ((I32, 12), (U8, 20)):
            for x in (ic.frames(rng, 1, 1500), ic.frames(rng, 3, 260)):
                for poke, at in ((32768, 0), (-32768, 1), (-32768, 0), (32768, 1), (40000, 0)):
                    h = ic.taps(rng, 9)
                    h[3, at] = poke
                    _check(x, h, U, frac, 32, stage, route=ic.GENERIC64, what=("a part of", poke, U, stage))
                h = ic.taps(rng, 9)
                h[3] = (32767, -32767)
                _check(x, h, U, frac, 32, stage, route=ic.FAST if 2 <= U <= 16 and stage == I32 else ic.GENERIC32,
                       what=("parts of +-32767", U, stage))
                _check(x, ic.taps(rng, 16), U, 32, 32, stage, route=ic.GENERIC64, what=("frac 32", U, stage))
                _check(x, ic.taps(rng, 7), U, frac, 32, stage, x_lead=2, route=ic.GENERIC64, what=("x % 4 == 2", U, stage))


def test_generic32_routes():
    rng = np.random.default_rng(62)
    g32 = ic.GENERIC32
    for U in (2, 3, 16):
        L = ic.fast_max_taps(U) + 1
        _check(ic.frames(rng, 1, 1501), ic.taps(rng, L), U, route=g32, what=("one tap too many", L, U))
        _check(ic.frames(rng, 3, 260), ic.taps(rng, 140), U, route=g32, what=("140 taps, rows", U))
        _check(ic.frames(rng, 2, 260), ic.taps(rng, 9, -40, 41), U, 6, 32, U8, route=g32, what=("u8 stage", U))
        _check(ic.frames(rng, 7, 3), ic.taps(rng, 64), U, route=g32, what=("rows of 3 frames", U))
        _check(ic.frames(rng, 5, 257), ic.taps(rng, 5), U, 31, 24, route=g32, what=("odd rows", U))
    for U in (1, 17, 40):
        for x in (ic.frames(rng, 1, 777), ic.frames(rng, 4, 260), ic.frames(rng, 3, 258), ic.frames(rng, 2, 5)):
            for L in (1, 16, 64, 129):
                _check(x, ic.taps(rng, L), U, route=g32, what=("rate", U, L, x.shape))




def test_generic128_route():
    """needs_wide: 2^16 + 9 complex taps of +-(2^31 - 1) make sum(|hr| + |hi|) * 32768 pass 2^63, so the
    kernel sums in 128 bits.  The reference is want_loop (unbounded Python ints), the only one that
    holds whatever a sum reaches; its loop is as long as the row, whatever the tap count."""
    rng = np.random.default_rng(63)
    L = (1 << 16) + 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert ic.sum_can_pass_2_63(hq)
    x = _runs(rng, 2, 40)
    for U, frac, acc, stage in ((3, 30, 64, I32), (2, 45, 80, U8), (1, 30, 64, I32), (17, 36, 64, I32)):
        ref = ic.want_loop(x, hq, U, frac, acc, stage)
        _check(x, hq, U, frac, acc, stage, ref=ref, route=ic.GENERIC128, what=("wide", U, frac, acc))


# ---- 6. identities on the device -------------------------------------------------------------------
def test_up_1_is_the_full_rate_filter():
    rng = np.random.default_rng(64)
    for L, frac, acc, stage in ((9, 12, 32, I32), (64, 3, 24, I32), (66, 12, 32, I32), (5, 20, 40, I32), (7, 6, 32, U8)):
        x = ic.frames(rng, 3, 1030)
        hq = ic.taps(rng, L, -40, 41) if stage == U8 else ic.taps(rng, L)
        _check(x, hq, 1, frac, acc, stage, what=("U = 1", L))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, 1, frac, acc, stage)
        full = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage)
        assert got.dtype == full.dtype and torch.equal(got, full), ("U = 1", L)


def test_real_taps_equal_the_real_interpolator():
    rng = np.random.default_rng(65)
    for L, U, frac, acc, stage in ((9, 4, 12, 32, I32), (64, 2, 8, 24, I32), (128, 16, 12, 32, I32), (140, 3, 12, 32, I32),
                                   (5, 17, 12, 40, I32), (7, 3, 6, 32, U8)):
        x = ic.frames(rng, 4, 516)
        hq = ic.taps(rng, L, -40, 41) if stage == U8 else ic.taps(rng, L)
        hq[:, 1] = 0
        _check(x, hq, U, frac, acc, stage, what=("real taps", L, U))
        xd = torch.from_numpy(x).to(DEV)
        got = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, U, frac, acc, stage)
        real = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq[:, 0], U, frac, acc, stage, 2)
        assert got.dtype == real.dtype and torch.equal(got, real), ("real taps", L, U)


def test_up_then_down_converter():
    """The down-converter at decim = U, phase = 0 over this call's output (which fits int16 here) equals
    the full-rate complex filter of the stuffed signal, filtered again and sliced the same way."""
    rng = np.random.default_rng(66)
    for U, L in ((2, 33), (3, 16), (16, 128)):
        x = ic.frames(rng, 4, 516)
        h, g = ic.taps(rng, L, -200, 201), ic.taps(rng, 24)
        xd = torch.from_numpy(x).to(DEV)
        up = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, h, U, 14)
        assert tuple(cinterp.last_launch()) == (ic.FAST, ic.bucket(L, U))
        full = torch_cplx.fir1d_fixed_rows_cplx_dev(torch.from_numpy(ic.stuffed(x, U)).to(DEV), h, 14)
        assert torch.equal(up, full)
        assert int(up.abs().max()) < 32768  # at most 17 taps meet a frame: 17 * 2 * 200 * 32768 / 2^14
        down = torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(up.to(torch.int16), g, U, 0)
        again = torch_cplx.fir1d_fixed_rows_cplx_dev(full.to(torch.int16), g)
        assert torch.equal(down.view(4, 516, 2), again.view(4, 516 * U, 2)[:, ::U])


# ---- 7. alignment ------------------------------------------------------------------------------------
def test_y_at_every_int32_offset_and_x_at_16_byte_offsets():
    rng = np.random.default_rng(70)
    x, x1, hq = ic.frames(rng, 4, 516), ic.frames(rng, 1, 2 * F + 37), ic.taps(rng, 24)
    for U in (2, 3, 16):
        ref, ref1 = ic.want(x, hq, U), ic.want(x1, hq, U)
        want = (ic.FAST, ic.bucket(24, U))
        for y_lead in (0, 4, 8, 12, 36):
            for x_lead in (0, 16, 48):
                assert _check(x, hq, U, ref=ref, x_lead=x_lead, y_lead=y_lead, what=("rows", U, x_lead, y_lead)) == want
            assert _check(x1, hq, U, ref=ref1, x_lead=32, y_lead=y_lead, what=("one row", U, y_lead)) == want
        for x_lead in (4, 8, 12):  # x off 16 bytes: the generic kernel, the same values
            _check(x, hq, U, ref=ref, x_lead=x_lead, y_lead=x_lead, route=ic.GENERIC32, what=("x off 16", U, x_lead))
            _check(x1, hq, U, ref=ref1, x_lead=x_lead, route=ic.GENERIC32, what=("one row, x off 16", U, x_lead))
        for width in (513, 514, 515):  # rows that do not start as x does
            _check(ic.frames(rng, 3, width), hq, U, route=ic.GENERIC32, what=("rows of", width, U))


# ---- 8. entry behaviour --------------------------------------------------------------------------------
def test_out_is_written_in_place():
    rng = np.random.default_rng(71)
    x, hq = ic.frames(rng, 4, 516), ic.taps(rng, 24)
    ref = ic.want(x, hq, 5)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.full((4, 2 * 516 * 5), -7, dtype=torch.int32, device=DEV)
    ptr = out.data_ptr()
    got = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, torch_cinterp.CplxTaps(hq), 5, out=out)
    assert got is out and out.data_ptr() == ptr
    _same(out.cpu().numpy(), ref, "out=")
    fresh = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd.reshape(2, 2, -1), hq, 5)
    assert fresh.shape == (2, 2, out.shape[1]) and torch.equal(fresh.reshape(4, -1), out)
    for bad in (torch.empty((4, out.shape[1] + 2), dtype=torch.int32, device=DEV), out.to(torch.int64), out.cpu()):
        with pytest.raises(fir_hip.FirHipError):
            torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, 5, out=bad)
    big = torch.zeros(4096, dtype=torch.int16, device=DEV)
    with pytest.raises(fir_hip.FirHipError, match="overlap"):  # 32 frames of x inside the bytes a U = 2 call writes
        torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(big[:64].view(1, 64), hq, 2, out=big.view(torch.int32)[8:136].view(1, 128))
    with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):
        torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, 0)


def test_caller_stream():
    rng = np.random.default_rng(72)
    x, hq = ic.frames(rng, 2, 4096), ic.taps(rng, 33)
    xd = torch.from_numpy(x).to(DEV)
    yd = torch.zeros((2, 2 * 4096 * 3), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    out = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, hq, 3, out=yd, stream=side)
    assert out is yd and tuple(cinterp.last_launch()) == (ic.FAST, ic.bucket(33, 3))
    side.synchronize()  # that stream only
    _same(yd.cpu().numpy(), ic.want(x, hq, 3), "side stream")


def _capture_and_replay(rows, width, U, taps, want_route):
    s = torch.cuda.Stream(device=DEV)
    x = torch.zeros((rows, 2 * width), dtype=torch.int16, device=DEV)  # static input and output
    y = torch.empty((rows, 2 * width * U), dtype=torch.int32, device=DEV)
    assert ic.predicted_route(x.data_ptr(), y.data_ptr(), rows, width, taps.h, U) == want_route
    with torch.cuda.stream(s):  # warm the entry outside the capture (a generic call's table is uploaded here)
        torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, taps, U, out=y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(x, taps, U, out=y)
    assert tuple(cinterp.last_launch()) == want_route
    torch.cuda.synchronize()
    for seed in (1, 2):
        xh = ic.frames(np.random.default_rng(seed), rows, width)
        x.copy_(torch.from_numpy(xh))
        y.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(y.cpu().numpy(), ic.want(xh, taps.h, U), ("replay", seed, want_route))


def test_fast_path_is_captured_once_and_replayed():
    """The fast path allocates nothing and reads no device table: one launch captured on a side stream
    in a graph of that single kernel, replayed twice on input changed in place."""
    rng = np.random.default_rng(73)
    _capture_and_replay(3, 2052, 4, torch_cinterp.CplxTaps(ic.taps(rng, 48)), (ic.FAST, ic.bucket(48, 4)))


def test_warmed_up_generic_call_is_captured_too():
    rng = np.random.default_rng(74)
    _capture_and_replay(3, 1030, 4, torch_cinterp.CplxTaps(ic.taps(rng, 48)), (ic.GENERIC32, 0))


def test_host_entry_agrees_with_the_device_entry():
    rng = np.random.default_rng(75)
    for rows, width, L, U, frac, acc, stage in ((3, 516, 33, 3, 12, 32, I32), (1, 2101, 128, 16, 12, 24, I32),
                                                (2, 258, 9, 2, 6, 32, U8), (2, 300, 70, 5, 20, 40, I32), (4, 6, 5, 8, 12, 32, I32)):
        x = ic.frames(rng, rows, width)
        hq = ic.taps(rng, L, -40, 41) if stage == U8 else ic.taps(rng, L)
        host = fir_hip.fir1d_fixed_rows_cplx_interp(x, hq, U, frac, acc, stage)
        launched = tuple(cinterp.last_launch())
        # the host form's device buffers come from hipMalloc: 16-byte aligned
        assert launched == ic.predicted_route(0, 0, rows, width, hq, U, frac, acc, stage), (rows, width, L, U)
        dev = torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(torch.from_numpy(x).to(DEV), hq, U, frac, acc, stage)
        assert np.array_equal(host, dev.cpu().numpy())
        _same(host, ic.want(x, hq, U, frac, acc, stage), ("host", rows, width, L, U))
    out = np.empty((3, 5, 2 * 40 * 3), np.int32)
    x = ic.frames(rng, 15, 40).reshape(3, 5, 80)
    hq = ic.taps(rng, 5)
    assert cinterp.fir1d_fixed_rows_cplx_interp(x, hq, 3, out=out) is out
    _same(out.reshape(15, -1), ic.want(x.reshape(15, 80), hq, 3), "host out=")


# ---- 9. random cases ---------------------------------------------------------------------------------
@settings(max_examples=60, **SETTINGS)
@given(ic.property_case())
def test_random_cases_vs_oracle(case):
    why, c = case
    x = rc.samples(c)
    hq = np.asarray(c.hq, dtype=np.int64)
    route, _ = _check(x, hq, c.up, c.frac, c.acc, c.stage, x_lead=c.x_lead, y_lead=c.y_lead, what=(why, c))
    assert (route == ic.FAST) == (why == ""), (why, c, route)
