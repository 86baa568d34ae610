"""GPU: the rational U/D resampling 1-D FIR (fir_resample_rows_dev through
torch_resample.fir1d_fixed_rows_resample_dev).

The reference for every value is the committed C oracle at full rate on the NumPy zero-stuffed
signal, viewed as (rows, width * U, ch) and sliced [:, phase::D]:

    xu = zeros(rows, width * U, ch); xu[:, ::U] = x
    c_oracle().fir1d_rows(xu, hq, frac, acc, stage, channels=ch).reshape(rows, width * U, ch)[:, phase::D]

so every comparison is np.array_equal, no tolerance.  The full-rate result does not depend on D or
phase: it is computed once per (x, hq) and sliced for every phase.

Geometry of the fast kernel (header comment of csrc/fir1d_resample.hip).  A period is U output
frames = D input frames.  A workgroup owns P periods of one row, P = 256 doubled until
P * D * in_size >= 4096; it works through them in tiles of T periods, T = P halved while
T * U * channels * out_size exceeds 16 KiB, at least 256; a tile is computed in passes of 512
periods, two per lane.  So a pass is 512 U output frames, a tile T U, a workgroup P U, and the rows
whose last output falls just before, at or past each of those boundaries are 512 D, T D and P D
input frames wide, one less and one more.  The fast kernel runs when resample_path_ok holds
(2 <= U, D <= 16, taps within int16 and ceil(L / U) <= 64, acc_bits <= 32, frac_bits <= 31, u8 x 1
channel or int16 x 1 | 2, x 16-byte aligned (u8: 8), one row or rows of a multiple of 8 samples; y at
any element address); U = 1 and D = 1 are forwarded to the decimator and the interpolator; every
other call takes the generic kernel.  No test here provokes a fault: all buffers are in bounds, the
guarded cases sit inside one allocation.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
import torch_resample_cases as rc
from fir_hip import torch_interp, torch_ops, torch_resample
from guarded import guarded_input, guarded_output
# the reference above, stated once for the grid and the property tests
from rate_property_cases import resample_slice as _slice, resample_up as _up, resample_want as _want

DEV = torch.device("cuda:0")
PASS = 512  # kResPass: periods the workgroup's lanes cover at once, two each

# name -> (sample dtype, out_stage, channels)
CONFIGS = {
    "u8_u8": (np.uint8, fir_hip.OUT_U8_SAT, 1),
    "u8_i32": (np.uint8, fir_hip.OUT_I32, 1),
    "i16_u8": (np.int16, fir_hip.OUT_U8_SAT, 1),
    "i16_i32": (np.int16, fir_hip.OUT_I32, 1),
    "c16_i32": (np.int16, fir_hip.OUT_I32, 2),
}
# coprime both ways, common factors, U | D and D | U
PAIRS = [(2, 3), (3, 2), (5, 3), (3, 5), (16, 15), (15, 16), (7, 16), (16, 7), (4, 6), (6, 4), (16, 16), (2, 2), (2, 16),
         (16, 2), (8, 4)]


def _geom(cfg, U, D):
    """(P, T) of fir1d_resample_kernel: periods per workgroup and per tile."""
    dtype, stage, ch = CONFIGS[cfg]
    P = 256
    while P * D * np.dtype(dtype).itemsize < 4096:
        P *= 2
    T = P
    while T > 256 and T * U * ch * (4 if stage == fir_hip.OUT_I32 else 1) > 16384:
        T //= 2
    return P, T


def _is_fast(xd, dtype, shape, ch, U, D, hq, acc=32, frac=12):
    """resample_path_ok, from the documented conditions."""
    aligned = xd.data_ptr() % (8 if dtype == np.uint8 else 16) == 0
    rows_ok = shape[0] == 1 or (shape[1] * ch) % 8 == 0
    taps_ok = -(-len(hq) // U) <= 64 and min(hq) >= -32768 and max(hq) <= 32767
    return (aligned and rows_ok and taps_ok and 2 <= U <= 16 and 2 <= D <= 16 and acc <= 32 and frac <= 31
            and (ch == 1 or (ch == 2 and dtype == np.int16)))


def _samples(rng, dtype, rows, width, ch):
    lo, hi = (0, 256) if dtype == np.uint8 else (-32768, 32768)
    return rng.integers(lo, hi, (rows, width * ch), dtype=dtype)


def _same(got, want, U, D, phase, ch, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        m = k // ch
        raise AssertionError(f"{what}: {len(bad)} of {want.size} outputs differ; the first at row {r}, output frame {m} "
                             f"(period {m // U}, q {m % U}, frame {m * D + phase} of the interpolated row), channel "
                             f"{k % ch}: {got[r, k]} != {want[r, k]}")


def _run(xd, hq, U, D, phase, frac, acc, stage, ch, **kw):
    """The device entry, its launch log held against _is_fast (U == 1 and D == 1 are forwarded to the
    decimator and the interpolator; an empty output launches nothing)."""
    with fir_hip.launch_log() as log:
        y = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq, U, D, phase, frac, acc, stage, ch, **kw)
    ks = [l.kernel for l in log]
    dtype = np.uint8 if xd.dtype == torch.uint8 else np.int16
    if y.numel() == 0:
        assert ks == [], ks
    elif U == 1 or D == 1:
        assert len(ks) == 1 and ks[0].startswith("fir1d_decim" if U == 1 else "fir1d_interp"), (U, D, ks)
    elif _is_fast(xd, dtype, (xd.shape[0], xd.shape[1] // ch), ch, U, D, [int(v) for v in np.asarray(hq).reshape(-1)], acc, frac):
        assert ks == ["fir1d_resample_kernel"], (U, D, len(hq), ks)
    else:
        assert ks == ["fir1d_resample_generic_kernel"], (U, D, len(hq), ks)
    return y.cpu().numpy()


def _check(x, hq, U, D, phases, frac, acc, stage, ch, what, xd=None):
    rows, rowlen = x.shape
    up = _up(x, hq, U, frac, acc, stage, ch)
    xd = torch.from_numpy(x).to(DEV) if xd is None else xd
    for phase in phases:
        want = _slice(up, D, phase)
        assert want.shape == (rows, fir_hip.resample_out_width(rowlen // ch, U, D, phase) * ch), (what, phase)
        _same(_run(xd, hq, U, D, phase, frac, acc, stage, ch), want, U, D, phase, ch, (what, phase))


# ---- 1. period, tile and row edges, fast kernel ------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("U,D", PAIRS, ids=[f"{u}over{d}" for u, d in PAIRS])
def test_fast_kernel_period_tile_and_row_edges(U, D, cfg):
    """Rows that end one frame before, at and one frame past the end of a pass, a tile and a
    workgroup, multi-row shapes, and rows narrower than a window or a period, for every phase kind
    and filter length.  The two longest filters (64 U and 64 U - 1 taps) run on the workgroup
    edges, which contain every pass and tile of a workgroup, and on the narrow rows."""
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(1000 * U + 10 * D + len(cfg))
    P, T = _geom(cfg, U, D)
    wg = [(1, P * D - 1), (1, P * D), (1, P * D + 1)]
    edges = [(1, w + d) for w in sorted({PASS * D, T * D}) for d in (-1, 0, 1)]
    edges = [s for s in edges if s not in wg]
    # (1, 1): phase >= width * U is an empty output for the late phases
    rows_ = [(3, 8), (5, 1032), (2, T * D + 8), (1, D - 1), (1, 1), (4, 8)]
    phases = sorted({0, D - 1, D // 2})
    hold = {s: _samples(rng, dtype, s[0], s[1], ch) for s in wg + edges + rows_}
    dev = {s: torch.from_numpy(v).to(DEV) for s, v in hold.items()}
    for L in sorted({1, 2, U - 1, U, U + 1, 31, 128, 129, 64 * U, 64 * U - 1}):
        hq = rng.integers(-2000, 2001, L)
        long = L > 129
        for s in wg + ([(1, D - 1), (4, 8), (3, 8)] if long else edges + rows_):
            assert _is_fast(dev[s], dtype, s, ch, U, D, hq) == (-(-L // U) <= 64)  # 129 taps at U = 2: generic
            _check(hold[s], hq, U, D, phases, 12, 32, stage, ch, (U, D, L, s, cfg), xd=dev[s])


# ---- 2. generic kernel branches -------------------------------------------------------------
def _generic_cases():
    c = []
    for U, D in ((17, 3), (3, 17), (64, 5), (5, 64), (1000, 7), (7, 1000), (17, 17), (1000, 64)):
        for L in (5, 129):
            c.append((f"U{U}_D{D}_L{L}", dict(U=U, D=D, L=L, shape=(3, 67) if U == 1000 else (3, 1061))))
    for L in (257, 260):  # ceil(L / U) = 65: one tap per phase too many for the fast kernel
        c.append((f"L{L}_U4_D3", dict(U=4, D=3, L=L, cfg="u8_u8", shape=(2, 1064))))
        c.append((f"L{L}_U4_D3_c16", dict(U=4, D=3, L=L, cfg="c16_i32", shape=(2, 1064))))
    c.append(("channels3", dict(U=4, D=3, L=9, ch=3)))
    c.append(("channels3_D16", dict(U=3, D=16, L=33, ch=3, shape=(3, 257))))
    c.append(("channels2_u8", dict(U=4, D=3, L=9, ch=2, cfg="u8_i32")))
    c.append(("acc40_u8", dict(U=2, D=3, L=5, acc=40, frac=33, cfg="u8_i32")))
    c.append(("acc48", dict(U=4, D=3, L=9, acc=48, frac=20)))
    c.append(("acc64", dict(U=3, D=2, L=31, acc=64, frac=12)))
    c.append(("acc33", dict(U=4, D=6, L=9, acc=33, frac=12)))
    c.append(("frac32", dict(U=4, D=3, L=9, acc=32, frac=32)))
    c.append(("x_off_2", dict(U=4, D=3, L=9, lead=2)))
    c.append(("x_off_8_i16", dict(U=3, D=4, L=9, lead=8)))
    c.append(("x_off_4_u8", dict(U=2, D=3, L=5, lead=4, cfg="u8_u8")))
    c.append(("x_off_2_complex", dict(U=8, D=5, L=64, lead=2, cfg="c16_i32")))
    c.append(("ragged_rows", dict(U=4, D=3, L=9, shape=(5, 1031))))
    c.append(("ragged_rows_u8", dict(U=3, D=2, L=5, shape=(5, 1031), cfg="u8_u8")))
    c.append(("tap_above_int16", dict(U=4, D=3, L=9, big_tap=32768)))
    c.append(("tap_below_int16", dict(U=3, D=2, L=9, big_tap=-32769)))
    c.append(("U_above_L_empty_phases", dict(U=700, D=3, L=9, shape=(6, 50))))
    c.append(("U_above_L_and_width_D_above_row", dict(U=20, D=2000, L=9, shape=(6, 50))))
    return c


@pytest.mark.parametrize("name,case", _generic_cases(), ids=[n for n, _ in _generic_cases()])
def test_generic_kernel_branches(name, case):
    dtype, stage, ch = CONFIGS[case.get("cfg", "i16_i32")]
    ch = case.get("ch", ch)
    U, D, L = case["U"], case["D"], case["L"]
    rng = np.random.default_rng(sum(map(ord, name)))  # a seed that does not change from run to run
    rows, width = case.get("shape", (3, 1061))
    x = _samples(rng, dtype, rows, width, ch)
    hq = rng.integers(-2000, 2001, L)
    if "big_tap" in case:
        hq[L // 2] = case["big_tap"]
    frac, acc = case.get("frac", 12), case.get("acc", 32)
    if "lead" in case:
        xd = guarded_input(torch.from_numpy(x), lead_bytes=case["lead"], device=DEV)
        assert xd.data_ptr() % 16 == case["lead"]
    else:
        xd = torch.from_numpy(x).to(DEV)
    assert not _is_fast(xd, dtype, (rows, width), ch, U, D, hq, acc, frac)
    _check(x, hq, U, D, sorted({0, D - 1, D // 2}), frac, acc, stage, ch, name, xd=xd)


def test_generic_kernel_wide_sums():
    """needs_wide: 2^17 + 9 taps of +-(2^31 - 1) make sum|h| * 32768 pass 2^63, so the generic
    kernel sums in 128 bits; the samples are small (|x| <= 100), so every true sum stays far
    below 2^63 and the C oracle's 64-bit sums are exact."""
    rng = np.random.default_rng(63)
    L = (1 << 17) + 9
    hq = np.where(rng.integers(0, 2, L) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert int(np.abs(hq).sum()) * 32768 >= 1 << 63
    x = rng.integers(-100, 101, (1, 1500), dtype=np.int16)
    for frac, acc, stage in ((30, 64, fir_hip.OUT_I32), (40, 80, fir_hip.OUT_U8_SAT)):
        _check(x, hq, 3, 2, (0, 1), frac, acc, stage, 1, ("wide", frac, acc))


# ---- 3. forwarding ------------------------------------------------------------------------------
def test_up_1_and_decim_1_are_the_decimator_and_the_interpolator():
    rng = np.random.default_rng(11)
    for cfg, (dtype, stage, ch) in CONFIGS.items():
        x = _samples(rng, dtype, 5, 1032, ch)
        xd = torch.from_numpy(x).to(DEV)
        for L in (5, 31, 129):
            hq = rng.integers(-2000, 2001, L)
            for D, phase in ((4, 1), (3, 2), (17, 0)):
                dec = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq, D, phase, 12, 32, stage, ch)
                got = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq, 1, D, phase, 12, 32, stage, ch)
                assert got.shape == dec.shape and torch.equal(got, dec), (cfg, L, D, phase)
            for U in (4, 3, 17):
                itp = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, U, 12, 32, stage, ch)
                got = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq, U, 1, 0, 12, 32, stage, ch)
                assert got.shape == itp.shape and torch.equal(got, itp), (cfg, L, U)
            full = torch_ops.fir1d_fixed_rows_dev(xd, hq, 12, 32, stage, ch)
            got = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq, 1, 1, 0, 12, 32, stage, ch)
            assert got.shape == full.shape and torch.equal(got, full), (cfg, L)


# ---- 4. arithmetic extremes, both kernels -----------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("U,D,L", [(2, 3, 128), (3, 2, 64), (16, 15, 1024), (8, 5, 5), (17, 3, 64)], ids=lambda v: str(v))
def test_arithmetic_extremes(U, D, L, cfg):
    """Taps at -32768 / 32767 against samples at the ends of their range: the 32-bit accumulator
    wraps many times over and v_dot2 must wrap, not saturate.  (17, 3, 64) runs the generic kernel."""
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(U * 1000 + L)
    lo, hi = (0, 255) if dtype == np.uint8 else (-32768, 32767)
    rows, width = 2, 264  # more than the 64 frames of the longest window; rows of a multiple of 8 samples
    x = np.where(rng.integers(0, 2, (rows, width * ch)) == 0, lo, hi).astype(dtype)
    x[0, : 80 * ch] = hi  # runs of one sign, so whole windows add up
    x[1, -80 * ch:] = lo
    xd = torch.from_numpy(x).to(DEV)
    taps = [np.where(rng.integers(0, 2, L) == 0, -32768, 32767), np.full(L, 32767), np.full(L, -32768)]
    phase = D // 2
    for hq in taps:
        assert _is_fast(xd, dtype, (rows, width), ch, U, D, hq) == (U <= 16)
        for acc in (8, 16, 24, 32):
            for frac in (1, 12, 31):
                for st in (fir_hip.OUT_U8_SAT, fir_hip.OUT_I32):
                    want = _want(x, hq, U, D, phase, frac, acc, st, ch)
                    got = _run(xd, hq, U, D, phase, frac, acc, st, ch)
                    _same(got, want, U, D, phase, ch, (U, D, L, cfg, int(hq[0]), acc, frac, st))


# ---- 5. guard bands -----------------------------------------------------------------------------
# shapes whose last tile is partial; x at leads on both sides of the fast path's alignment condition
# (16 bytes, u8: 8), y at every kind of lead: the fast kernel has no condition on y, its first and
# last 16-byte vector of a tile go out element by element
GUARDED = [
    # cfg, U, D, phase, L, (rows, width), x_lead, y_lead, fast
    ("u8_u8", 3, 2, 1, 15, (3, 4096 + 40), 8, 3, True),
    ("u8_i32", 5, 3, 0, 31, (1, 2048 * 3 + 13), 0, 4, True),
    ("i16_u8", 16, 15, 14, 1024, (2, 256 * 15 + 72), 16, 1, True),
    ("i16_i32", 2, 3, 2, 128, (1, 1024 * 3 + 7), 0, 12, True),
    ("c16_i32", 16, 7, 3, 33, (3, 512 * 7 + 20), 32, 8, True),
    ("i16_i32", 4, 6, 5, 9, (8, 512 * 6 + 8), 48, 0, True),
    ("i16_i32", 7, 16, 8, 100, (1, 700), 0, 4, True),
    # generic: a misaligned x, rows that are no multiple of 8 samples, a rate outside the fast path
    ("i16_i32", 4, 3, 1, 9, (3, 1031), 2, 4, False),
    ("u8_u8", 17, 5, 4, 300, (5, 1031), 1, 5, False),
    ("u8_u8", 3, 2, 0, 5, (3, 552), 4, 3, False),
    ("i16_i32", 3, 2, 1, 9, (2, 1032), 8, 12, False),
]


@pytest.mark.parametrize("cfg,U,D,phase,L,shape,x_lead,y_lead,fast", GUARDED)
def test_guard_bands(cfg, U, D, phase, L, shape, x_lead, y_lead, fast):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(U * 100 + D * 10 + L)
    x = _samples(rng, dtype, shape[0], shape[1], ch)
    hq = rng.integers(-2000, 2001, L)
    want = _want(x, hq, U, D, phase, 12, 32, stage, ch)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    assert xd.data_ptr() % 16 == x_lead % 16
    assert fast == _is_fast(xd, dtype, shape, ch, U, D, hq)
    assert shape[1] % (_geom(cfg, U, D)[1] * D) != 0  # the last tile is partial
    yd, check = guarded_output(want.shape, torch.uint8 if stage == fir_hip.OUT_U8_SAT else torch.int32,
                               lead_bytes=y_lead, device=DEV)
    assert yd.data_ptr() % 16 == y_lead
    out = torch_resample.fir1d_fixed_rows_resample_dev(xd, hq, U, D, phase, 12, 32, stage, ch, out=yd)
    assert out is yd
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), want, U, D, phase, ch, (cfg, U, D, L))
    check(f"{cfg} U={U} D={D}")


# ---- 6. one medium size per kernel family -----------------------------------------------------------
@pytest.mark.parametrize("cfg", ["i16_i32", "c16_i32"])
def test_medium_int16(cfg):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(22)
    x = _samples(rng, dtype, 1, 1 << 20, ch)
    _check(x, rng.integers(-3000, 3001, 33), 3, 2, (1,), 12, 32, stage, ch, cfg)


def test_medium_u8_rows():
    rng = np.random.default_rng(23)
    x = _samples(rng, np.uint8, 1024, 4096, 1)
    hq = [-64, -128, 0, 256, 640, 1024, 1408, 1600, 1408, 1024, 640, 256, 0, -128, -64]
    _check(x, hq, 3, 2, (0,), 12, 32, fir_hip.OUT_U8_SAT, 1, "u8 rows")


# ---- 7. graph capture -----------------------------------------------------------------------------
def test_fast_path_is_capturable():
    """The fast path allocates nothing and reads no device table: captured on one stream (a single
    linear chain, no parallel branches), replayed twice with x changed in place between replays."""
    rng = np.random.default_rng(6)
    U, D, phase, L = 3, 2, 1, 33
    hq = torch_ops.Taps(rng.integers(-3000, 3001, L))
    shapes = {"i16_i32": (1, 3 * 2048 + 40), "c16_i32": (2, 2048 + 16), "u8_u8": (8, 4096)}
    ow = {k: fir_hip.resample_out_width(w, U, D, phase) for k, (r, w) in shapes.items()}
    xs = {k: torch.zeros((r, w * CONFIGS[k][2]), dtype=torch.uint8 if CONFIGS[k][0] == np.uint8 else torch.int16,
                         device=DEV) for k, (r, w) in shapes.items()}
    ys = {k: torch.empty((r, ow[k] * CONFIGS[k][2]),
                         dtype=torch.uint8 if CONFIGS[k][1] == fir_hip.OUT_U8_SAT else torch.int32, device=DEV)
          for k, (r, w) in shapes.items()}
    for k in shapes:
        assert _is_fast(xs[k], CONFIGS[k][0], shapes[k], CONFIGS[k][2], U, D, hq.h)

    def step():
        for k in shapes:
            torch_resample.fir1d_fixed_rows_resample_dev(xs[k], hq, U, D, phase, 12, 32, CONFIGS[k][1], CONFIGS[k][2],
                                                         out=ys[k])

    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    torch.cuda.synchronize()
    for seed in (1, 2):
        r2 = np.random.default_rng(seed)
        host = {k: _samples(r2, CONFIGS[k][0], shapes[k][0], shapes[k][1], CONFIGS[k][2]) for k in shapes}
        for k in shapes:
            xs[k].copy_(torch.from_numpy(host[k]))  # in place: the graph holds the addresses
            ys[k].zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k in shapes:
            want = _want(host[k], hq.h, U, D, phase, 12, 32, CONFIGS[k][1], CONFIGS[k][2])
            _same(ys[k].cpu().numpy(), want, U, D, phase, CONFIGS[k][2], (seed, k))


# ---- 8. empty problems, out= reuse, refusals, the host entry -------------------------------------------
def test_empty_problems_and_out_reuse():
    hq = [-256, -1024, 6656, -1024, -256]
    f = torch_resample.fir1d_fixed_rows_resample_dev
    for shape, U, D, phase, ch in (((0, 64), 4, 3, 1, 1), ((5, 0), 4, 3, 0, 1), ((5, 0), 1, 1, 0, 1), ((4, 0), 16, 15, 14, 2),
                                   ((0,), 2, 3, 0, 1), ((0, 6), 1000, 7, 6, 3), ((5, 1), 3, 8, 3, 1), ((5, 2), 2, 16, 4, 2)):
        x = torch.zeros(shape, dtype=torch.int16, device=DEV)
        y = f(x, hq, U, D, phase, channels=ch)
        assert y.dtype == torch.int32 and y.numel() == 0
        assert tuple(y.shape) == tuple(shape[:-1]) + (fir_hip.resample_out_width(shape[-1] // ch, U, D, phase) * ch,)
    rng = np.random.default_rng(7)
    out = torch.empty((3, 1548), dtype=torch.int32, device=DEV)  # 1032 * 3 / 2
    for seed in (1, 2):  # the same out buffer, twice: nothing of the first call survives
        x = _samples(np.random.default_rng(seed), np.int16, 3, 1032, 1)
        got = f(torch.from_numpy(x).to(DEV), hq, 3, 2, out=out)
        assert got is out
        _same(out.cpu().numpy(), _want(x, hq, 3, 2, 0, 12, 32, fir_hip.OUT_I32, 1), 3, 2, 0, 1, ("reuse", seed))
    x = torch.from_numpy(_samples(rng, np.int16, 3, 1032, 1)).to(DEV)
    for bad in (torch.empty((3, 1548), dtype=torch.uint8, device=DEV), torch.empty((3, 1032), dtype=torch.int32, device=DEV),
                torch.empty((3, 1547), dtype=torch.int32, device=DEV), torch.empty((3, 3096), dtype=torch.int32, device=DEV),
                torch.empty((3, 1548), dtype=torch.int32)):
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            f(x, hq, 3, 2, out=bad)
    for U, D, phase, text in ((0, 2, 0, "up must be >= 1"), (-4, 2, 0, "up must be >= 1"), (3, 0, 0, "decim must be >= 1"),
                              (3, 2, 2, r"phase must be in \[0, decim\)"), (3, 2, -1, r"phase must be in \[0, decim\)")):
        with pytest.raises(fir_hip.FirHipError, match=text):
            f(x, hq, U, D, phase)
    # the host entry, through the same kernels: the fast one, and the generic one
    xh = _samples(rng, np.uint8, 7, 4096, 1)
    _same(fir_hip.fir1d_fixed_rows_resample(xh, hq, 8, 5, 2), _want(xh, hq, 8, 5, 2, 12, 32, fir_hip.OUT_U8_SAT, 1), 8, 5, 2, 1,
          "host fast")
    xc = _samples(rng, np.int16, 3, 515, 2)
    got = fir_hip.fir1d_fixed_rows_resample(xc, hq, 17, 3, 1, 14, 40, fir_hip.OUT_I32, channels=2)
    _same(got, _want(xc, hq, 17, 3, 1, 14, 40, fir_hip.OUT_I32, 2), 17, 3, 1, 2, "host generic")
    y = np.empty((7, 4096 * 3 // 2), np.uint8)
    assert fir_hip.fir1d_fixed_rows_resample(xh, hq, 3, 2, out=y) is y
    _same(y, _want(xh, hq, 3, 2, 0, 12, 32, fir_hip.OUT_U8_SAT, 1), 3, 2, 0, 1, "host out=")
    assert fir_hip.fir1d_fixed_rows_resample(np.zeros((4, 0), np.uint8), hq, 5, 3).shape == (4, 0)
    assert fir_hip.fir1d_fixed_rows_resample(np.zeros((4, 1), np.uint8), hq, 3, 8, 5).shape == (4, 0)


@pytest.mark.parametrize("case", rc.CASES, ids=[c.id for c in rc.CASES])
def test_contract_case_on_device_tensors(case, monkeypatch):
    """tests/torch_resample_cases.py on real cuda:0 tensors, still against the stub library: nothing
    is launched, a refused case never reaches the real library."""
    rc.run(case, rc.Maker(standin=False), torch_resample, monkeypatch)
