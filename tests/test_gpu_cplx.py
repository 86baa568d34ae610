"""GPU: the complex-tap FIR (fir_cplx_rows_dev through torch_cplx.fir1d_fixed_rows_cplx_dev).

The reference for every value is tests/cplx_ref.py's ``want``: two real filters of the committed C
oracle over the flattened row (tests/test_cplx_ref.py holds it against a direct Python-int loop), so
every comparison is np.array_equal, no tolerance.

Geometry of the fast kernel (header comment of csrc/fir1d_cplx.hip).  The frames of all rows are one
flat stream.  A lane owns V = 4 consecutive output frames (a lane group), a wave 256 (the unit of
the LDS output stage: a partial wave stores per lane), a workgroup a tile of 1024, staged with 32
frames before and 36 after it.  Filters are zero-padded to LP in {2, 4, 6, 8, 12, 16, 24, 32, 48, 64}.
So the single rows here are 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048 and 2049 frames
wide; the multi-row shapes of the fast path have rows of a multiple of 4 frames, down to rows far
narrower than a window (4 and 8 frames under 64 taps); rows of 4k + 2 frames end inside a lane's
vector and take the generic kernel.  The fast kernel runs when cplx_path_ok holds (at most 64 taps,
both parts within [-32767, 32767], acc_bits <= 32, frac_bits <= 31, OUT_I32, x and y 16-byte aligned,
one row or rows of a multiple of 4 frames); taps whose every hi is 0 are forwarded to the real
two-channel call; every other call takes a generic kernel: its 32-bit v_dot2 form where only the tap
count, an alignment, the row length or the u8 stage keeps the call off the fast path (a workgroup
of 256 frames inside one row walks its taps wave-uniformly, the ones at a row's ends per lane: rows
of 1028 and 1030 frames have both), its 64-bit form otherwise.  No test here provokes a fault: all
buffers are in bounds, the guarded cases sit inside one allocation.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
import torch_cplx_cases as cc
from cplx_ref import want as _ref
from fir_hip import torch_cplx, torch_ops
from guarded import guarded_input, guarded_output

DEV = torch.device("cuda:0")
VEC, WAVE, TILE, MAX_TAPS = 4, 256, 1024, 64  # kCxVec, kWave * kCxVec, kCxTile, kCxMaxTaps
BUCKETS = (2, 4, 6, 8, 12, 16, 24, 32, 48, 64)
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT


def _is_fast(xd, yd, shape, hq, acc=32, frac=12, stage=I32):
    """cplx_path_ok, from the documented conditions (for taps that are not all real)."""
    h = np.asarray(hq, dtype=object).reshape(-1, 2)
    taps_ok = len(h) <= MAX_TAPS and all(-32767 <= int(v) <= 32767 for v in h.reshape(-1))
    aligned = xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    rows_ok = shape[0] == 1 or shape[1] % VEC == 0
    return taps_ok and aligned and rows_ok and acc <= 32 and frac <= 31 and stage == I32


def _route(log, xd, yd, shape, hq, acc, frac, stage, what):
    """The call's launch log against _is_fast: the LDS kernel, else a generic one; taps that are all
    real are forwarded to the two-channel row entry, and an empty call launches nothing."""
    ks = [l.kernel for l in log]
    h = np.asarray(hq, dtype=object).reshape(-1, 2)
    if shape[0] * shape[1] == 0:
        assert ks == [], (what, ks)
    elif all(int(v) == 0 for v in h[:, 1]):
        assert len(ks) == 1 and not ks[0].startswith("fir1d_cplx"), (what, ks)
    elif _is_fast(xd, yd, (shape[0], shape[1] // 2), hq, acc, frac, stage):
        assert ks == ["fir1d_cplx_kernel"], (what, ks)
    else:
        assert len(ks) == 1 and ks[0] in ("fir1d_cplx_generic_kernel", "fir1d_cplx_generic32_kernel"), (what, ks)


def _frames(rng, rows, width):
    return rng.integers(-32768, 32768, (rows, 2 * width), dtype=np.int16)


def _taps(rng, L, lo=-3000, hi=3001):
    h = rng.integers(lo, hi, (L, 2))
    h[L // 2, 1] = 77  # never all real: the call must not be forwarded
    return h


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at row {r}, frame {k // 2} "
                             f"({'im' if k % 2 else 're'}): {got[r, k]} != {want[r, k]}")


def _check(x, hq, frac=12, acc=32, stage=I32, what="", fast=None, xd=None):
    xd = torch.from_numpy(x).to(DEV) if xd is None else xd
    yd = torch.empty(x.shape, dtype=torch.int32 if stage == I32 else torch.uint8, device=DEV)
    if fast is not None:
        assert _is_fast(xd, yd, (x.shape[0], x.shape[1] // 2), hq, acc, frac, stage) == fast, what
    with fir_hip.launch_log() as log:
        out = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage, out=yd)
    assert out is yd
    _route(log, xd, yd, x.shape, hq, acc, frac, stage, what)
    _same(yd.cpu().numpy(), _ref(x, hq, frac, acc, stage), what)


# ---- 1. lane-group, wave, tile and row edges, fast kernel ------------------------------------------
SINGLE = [VEC - 1, VEC, VEC + 1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
MULTI = [(3, 4), (5, 8), (300, 4), (130, 8), (7, 12), (5, 1028), (3, TILE), (2, TILE + 4), (9, 252), (4, 260)]


@pytest.mark.parametrize("L", [1, 2, 5, 16, 33, 63, 64])
def test_fast_kernel_lane_tile_and_row_edges(L):
    """Single rows that end one frame before, at and one frame past a lane group, a wave, a tile and
    two tiles; multi-row shapes of a multiple of 4 frames (rows of 4 and 8 frames are far narrower
    than a 64-tap window: a lane's window then spans many rows and keeps only its own); single rows
    narrower than the window (1, 2 and L - 1 frames)."""
    rng = np.random.default_rng(10 + L)
    hq = _taps(rng, L)
    for width in SINGLE + sorted({1, 2, max(1, L - 1)}):
        _check(_frames(rng, 1, width), hq, what=(L, 1, width), fast=True)
    for rows, width in MULTI:
        _check(_frames(rng, rows, width), hq, what=(L, rows, width), fast=True)


def test_every_tap_count_on_a_two_tile_row_and_on_rows():
    """Taps 1..64 on a row of two tiles and on 4 rows of 516 frames: every LP bucket, both parities of
    c = L // 2, the shift that keeps the centre frame, and the row mask under every window length."""
    rng = np.random.default_rng(2)
    x1, x4 = _frames(rng, 1, 2 * TILE), _frames(rng, 4, 516)
    d1, d4 = torch.from_numpy(x1).to(DEV), torch.from_numpy(x4).to(DEV)
    assert all(any(L <= b for b in BUCKETS) for L in range(1, MAX_TAPS + 1))
    for L in range(1, MAX_TAPS + 1):
        hq = _taps(rng, L)
        _check(x1, hq, what=(L, "two tiles"), fast=True, xd=d1)
        _check(x4, hq, what=(L, "rows"), fast=True, xd=d4)


# ---- 2. arithmetic extremes, fast kernel ------------------------------------------------------------
@pytest.mark.parametrize("acc", [16, 24, 31, 32])
def test_wrap_and_rounding_extremes(acc):
    """All -32768 samples against +-32767 taps: with 64 taps both sums pass 2^31 many times over, so
    the 32-bit accumulators wrap and v_dot2 must wrap, not saturate; frac_bits 1, 12 and 31."""
    rng = np.random.default_rng(acc)
    x = np.full((2, 2 * 264), -32768, np.int16)
    x[1, 2 * 100:] = rng.integers(-32768, 32768, 2 * 164)
    xd = torch.from_numpy(x).to(DEV)
    for L in (5, 64):
        for hq in (np.tile([[32767, 32767]], (L, 1)), np.tile([[32767, -32767]], (L, 1)), np.tile([[-32767, 32767]], (L, 1)),
                   np.where(rng.integers(0, 2, (L, 2)) == 0, -32767, 32767)):
            for frac in (1, 12, 31):
                _check(x, hq, frac, acc, what=(acc, L, frac, hq[0].tolist()), fast=True, xd=xd)


# ---- 3. the forward ----------------------------------------------------------------------------------
def test_real_taps_are_the_two_channel_real_call():
    rng = np.random.default_rng(3)
    for shape in ((1, 2 * TILE + 5), (5, 1028), (3, 1031)):
        x = _frames(rng, *shape)
        xd = torch.from_numpy(x).to(DEV)
        for L in (1, 5, 9, 33, 65):
            hr = rng.integers(-3000, 3001, L)
            hq = np.stack([hr, np.zeros(L, np.int64)], axis=1)
            for acc, frac, stage in ((32, 12, I32), (24, 1, I32), (40, 20, I32), (32, 12, U8)):
                real = torch_ops.fir1d_fixed_rows_dev(xd, hr, frac, acc, stage, channels=2)
                got = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage)
                assert got.dtype == real.dtype and torch.equal(got, real), (shape, L, acc, frac, stage)
                _same(got.cpu().numpy(), _ref(x, hq, frac, acc, stage), (shape, L, acc, frac, stage))


# ---- 4. generic kernel: each trigger alone ----------------------------------------------------------
def _generic_cases():
    c = [("part_minus_32768_hr", dict(L=9, poke=(4, 0, -32768))), ("part_minus_32768_hi", dict(L=9, poke=(0, 1, -32768))),
         ("tap_int32_sized", dict(L=9, poke=(3, 1, (1 << 31) - 1))), ("tap_32768", dict(L=9, poke=(8, 0, 32768))),
         ("taps_65", dict(L=65)), ("taps_200", dict(L=200)), ("acc_40", dict(L=9, acc=40)), ("acc_64", dict(L=33, acc=64)),
         ("acc_33", dict(L=9, acc=33)), ("frac_40", dict(L=9, frac=40)), ("frac_32", dict(L=9, frac=32)),
         ("stage_u8", dict(L=9, stage=U8)), ("stage_u8_acc_40", dict(L=5, stage=U8, acc=40, frac=20)),
         ("x_off_one_frame", dict(L=9, x_lead=4)), ("x_off_two_frames", dict(L=9, x_lead=8)),
         ("y_off_one_frame", dict(L=9, y_lead=8)), ("rows_4k_plus_2", dict(L=9, shape=(5, 1030))),
         ("rows_odd", dict(L=9, shape=(5, 1031))), ("rows_narrow_ragged", dict(L=64, shape=(40, 6)))]
    return c


@pytest.mark.parametrize("name,case", _generic_cases(), ids=[n for n, _ in _generic_cases()])
def test_generic_kernel_triggers(name, case):
    rng = np.random.default_rng(sum(map(ord, name)))
    rows, width = case.get("shape", (4, 1028))
    L, acc, frac, stage = case["L"], case.get("acc", 32), case.get("frac", 12), case.get("stage", I32)
    x = _frames(rng, rows, width)
    hq = _taps(rng, L)
    if "poke" in case:
        k, part, v = case["poke"]
        hq[k, part] = v
    xd = guarded_input(torch.from_numpy(x), lead_bytes=case.get("x_lead", 0), device=DEV)
    yd, check = guarded_output(x.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=case.get("y_lead", 0),
                               device=DEV)
    assert xd.data_ptr() % 16 == case.get("x_lead", 0) and yd.data_ptr() % 16 == case.get("y_lead", 0)
    assert not _is_fast(xd, yd, (rows, width), hq, acc, frac, stage)
    # the case's trigger is all that keeps it off the fast kernel: the call every case varies is fast
    x0 = guarded_input(torch.zeros((4, 2 * 1028), dtype=torch.int16), device=DEV)
    y0, _ = guarded_output((4, 2 * 1028), torch.int32, device=DEV)
    assert _is_fast(x0, y0, (4, 1028), _taps(rng, 9), 32, 12, I32)
    torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, frac, acc, stage, out=yd)
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), _ref(x, hq, frac, acc, stage), name)
    check(name)


@pytest.mark.parametrize("acc", [16, 24, 31, 32])
def test_generic_kernel_32_bit_form_extremes(acc):
    """The generic kernel's 32-bit form (int16-sized parts, acc_bits <= 32, frac_bits <= 31, x 4-byte
    aligned; here kept off the fast path by 65 and 200 taps, by rows of 4k + 2 frames and by the u8
    stage): all -32768 samples against +-32767 taps, so both sums pass 2^31 and must wrap."""
    rng = np.random.default_rng(200 + acc)
    x = np.full((3, 2 * 1030), -32768, np.int16)
    x[2, 2 * 400:] = rng.integers(-32768, 32768, 2 * 630)
    xd = torch.from_numpy(x).to(DEV)
    for L in (5, 65, 200):
        for hq in (np.tile([[32767, -32767]], (L, 1)), np.where(rng.integers(0, 2, (L, 2)) == 0, -32767, 32767)):
            for frac in (1, 31):
                _check(x, hq, frac, acc, what=(acc, L, frac), fast=False, xd=xd)
            _check(x, hq, 12, acc, U8, what=(acc, L, "u8"), fast=False, xd=xd)


def test_generic_kernel_x_at_an_odd_int16():
    """x two bytes off a dword: a frame is no aligned dword, so the 64-bit form runs whatever the taps."""
    rng = np.random.default_rng(77)
    x, hq = _frames(rng, 3, 1028), _taps(rng, 9)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=2, device=DEV)
    assert xd.data_ptr() % 4 == 2
    _check(x, hq, what="x % 4 == 2", fast=False, xd=xd)
    _check(x, _taps(rng, 70), 31, 24, what="x % 4 == 2, 70 taps", fast=False, xd=xd)


def test_generic_kernel_wide_sums():
    """needs_wide: 2^16 + 3 taps of +-(2^31 - 1) in both parts make sum(|hr| + |hi|) * 32768 pass
    2^63, so the generic kernel sums in 128 bits; the samples are small (|x| <= 100), so every true
    sum stays far below 2^63 and the C oracle's 64-bit sums are exact."""
    rng = np.random.default_rng(63)
    L = (1 << 16) + 3
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert int(np.abs(hq).sum()) * 32768 >= 1 << 63
    x = rng.integers(-100, 101, (1, 2 * 1500), dtype=np.int16)
    for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
        _check(x, hq, frac, acc, stage, what=("wide", frac, acc), fast=False)


# ---- 5. guard bands, fast kernel -------------------------------------------------------------------
GUARDED = [
    # L, (rows, width), x_lead, y_lead: leads that keep both 16-byte aligned; last tile / wave partial
    (5, (1, 2 * TILE + 13), 0, 0), (64, (1, TILE + 255), 16, 32), (33, (3, 1028), 32, 16), (64, (70, 4), 48, 0),
    (16, (1, 3), 0, 16), (12, (2, TILE), 0, 0),
]


@pytest.mark.parametrize("L,shape,x_lead,y_lead", GUARDED)
def test_guard_bands_fast(L, shape, x_lead, y_lead):
    rng = np.random.default_rng(L * 100 + shape[1])
    x, hq = _frames(rng, *shape), _taps(rng, L)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    yd, check = guarded_output(x.shape, torch.int32, lead_bytes=y_lead, device=DEV)
    assert _is_fast(xd, yd, shape, hq)
    out = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, out=yd)
    assert out is yd
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), _ref(x, hq), (L, shape))
    check(f"L={L} {shape}")


# ---- 6. one medium size, a caller stream, graph capture, the host entry ---------------------------------
def test_medium_row():
    rng = np.random.default_rng(22)
    _check(_frames(rng, 1, 1 << 20), _taps(rng, 33), what="2^20 frames", fast=True)


def test_caller_stream():
    rng = np.random.default_rng(23)
    x, hq = _frames(rng, 6, 4096), _taps(rng, 16)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to(DEV)
    s.synchronize()
    y = torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, stream=s)
    s.synchronize()
    _same(y.cpu().numpy(), _ref(x, hq), "stream")


def test_fast_path_is_capturable():
    """The fast path allocates nothing and reads no device table: one kernel captured on one stream
    (a single node, no parallel branches), replayed twice with x changed in place between replays."""
    rng = np.random.default_rng(6)
    hq = torch_cplx.CplxTaps(_taps(rng, 33))
    shape = (2, TILE + 16)
    xd = torch.zeros((shape[0], 2 * shape[1]), dtype=torch.int16, device=DEV)
    yd = torch.empty((shape[0], 2 * shape[1]), dtype=torch.int32, device=DEV)
    assert _is_fast(xd, yd, shape, hq.h)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, out=yd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq, out=yd)
    torch.cuda.synchronize()
    for seed in (1, 2):
        host = _frames(np.random.default_rng(seed), *shape)
        xd.copy_(torch.from_numpy(host))  # in place: the graph holds the addresses
        yd.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(yd.cpu().numpy(), _ref(host, hq.h), ("replay", seed))


def test_empty_problems_out_reuse_and_the_host_entry():
    hq = [[-256, 9], [6656, -3], [-1024, 70]]
    f = torch_cplx.fir1d_fixed_rows_cplx_dev
    for shape in ((0, 64), (5, 0), (0,), (3, 0, 8)):
        y = f(torch.zeros(shape, dtype=torch.int16, device=DEV), hq)
        assert y.dtype == torch.int32 and y.numel() == 0 and tuple(y.shape) == shape
    out = torch.empty((3, 2 * 1028), dtype=torch.int32, device=DEV)
    for seed in (1, 2):  # the same out buffer, twice: nothing of the first call survives
        x = _frames(np.random.default_rng(seed), 3, 1028)
        assert f(torch.from_numpy(x).to(DEV), hq, out=out) is out
        _same(out.cpu().numpy(), _ref(x, hq), ("reuse", seed))
    # the host entry, through the same kernels: the fast one, the generic one, the forward
    rng = np.random.default_rng(7)
    xh = _frames(rng, 7, 4096)
    _same(fir_hip.fir1d_fixed_rows_cplx(xh, hq), _ref(xh, hq), "host fast")
    xg = _frames(rng, 3, 515)
    _same(fir_hip.fir1d_fixed_rows_cplx(xg, hq, 14, 40, U8), _ref(xg, hq, 14, 40, U8), "host generic")
    y = np.empty(xh.shape, np.int32)
    assert fir_hip.fir1d_fixed_rows_cplx(xh, [[5, 0], [7, 0]], out=y) is y
    _same(y, fir_hip.fir1d_fixed_rows(xh, [5, 7], 12, 32, I32, channels=2), "host forward")
    assert fir_hip.fir1d_fixed_rows_cplx(np.zeros((4, 0), np.int16), hq).shape == (4, 0)
    x3 = _frames(rng, 6, 20).reshape(2, 3, 40)  # leading axes are rows
    _same(fir_hip.fir1d_fixed_rows_cplx(x3, hq).reshape(6, 40), _ref(x3.reshape(6, 40), hq), "host 3-d")


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_contract_case_on_device_tensors(case, monkeypatch):
    """tests/torch_cplx_cases.py on real cuda:0 tensors, still against the stub library: nothing is
    launched, a refused case never reaches the real library."""
    cc.run(case, cc.Maker(standin=False), torch_cplx, monkeypatch)
