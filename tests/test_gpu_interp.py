"""GPU: the interpolating 1-D FIR (fir_interp_rows_dev through torch_interp.fir1d_fixed_rows_interp_dev).

The reference for every value is the committed C oracle at full rate on the NumPy zero-stuffed
signal:

    xu = zeros(rows, width * U, ch); xu[:, ::U] = x
    c_oracle().fir1d_rows(xu, hq, frac, acc, stage, channels=ch)

so every comparison is np.array_equal, no tolerance.  T is the number of input frames in one tile
of the fast kernel and G its tiles per workgroup (header comment of csrc/fir1d_interp.hip: a
workgroup owns F = 4096 frames of u8 or 2048 of int16; T is F halved while T * U * channels *
out_size exceeds 16 KiB, at least 256; G = F / T; a tile is computed in passes of 512 frames); the
shapes are built around them so that passes, tiles and workgroups end exactly at, one short of and
one past a row's end.  The fast
kernel runs when interp_path_ok holds (2 <= U <= 16, L <= 128 taps within int16, acc_bits <= 32,
frac_bits <= 31, u8 x 1 channel or int16 x 1 | 2, x 16-byte aligned (u8: 8), one row or rows of a
multiple of 8 samples; y at any element address); every other call takes the generic kernel.  No
test here provokes a fault: all buffers are in bounds, the guarded cases sit inside one allocation.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
import torch_interp_cases as ic
from fir_hip import torch_interp, torch_ops
from guarded import guarded_input, guarded_output
from oracle import c_oracle
from rate_property_cases import interp_want as _want, stuff as _stuff  # the reference above, stated once

DEV = torch.device("cuda:0")
PASS = 512  # kIntPass: input frames the workgroup's lanes cover at once, two each

# name -> (sample dtype, out_stage, channels)
CONFIGS = {
    "u8_u8": (np.uint8, fir_hip.OUT_U8_SAT, 1),
    "u8_i32": (np.uint8, fir_hip.OUT_I32, 1),
    "i16_u8": (np.int16, fir_hip.OUT_U8_SAT, 1),
    "i16_i32": (np.int16, fir_hip.OUT_I32, 1),
    "c16_i32": (np.int16, fir_hip.OUT_I32, 2),
}


def _tile(cfg, U):
    """(T, G) of fir1d_interp_kernel for a configuration (csrc/fir1d_interp.hip, header comment)."""
    dtype, stage, ch = CONFIGS[cfg]
    F = 4096 // np.dtype(dtype).itemsize  # input frames per workgroup
    T = F
    while T > 256 and T * U * ch * (4 if stage == fir_hip.OUT_I32 else 1) > 16384:
        T //= 2
    return T, F // T


def _samples(rng, dtype, rows, width, ch):
    lo, hi = (0, 256) if dtype == np.uint8 else (-32768, 32768)
    return rng.integers(lo, hi, (rows, width * ch), dtype=dtype)


def _is_fast(xd, shape, ch, U, hq, acc, frac):
    """interp_path_ok, from the documented conditions (the module docstring, fir_launch.h)."""
    u8 = xd.dtype == torch.uint8
    h = [int(v) for v in np.asarray(hq, dtype=object).reshape(-1)]
    return (2 <= U <= 16 and len(h) <= 128 and min(h) >= -32768 and max(h) <= 32767 and acc <= 32 and frac <= 31
            and (ch == 1 or (ch == 2 and not u8)) and xd.data_ptr() % (8 if u8 else 16) == 0
            and (shape[0] == 1 or shape[1] % 8 == 0))


def _run(x, hq, U, frac, acc, stage, ch, **kw):
    """The device entry, its launch log held against _is_fast (an empty output launches nothing)."""
    xd = torch.from_numpy(x).to(DEV)
    with fir_hip.launch_log() as log:
        y = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, U, frac, acc, stage, ch, **kw)
    ks = [l.kernel for l in log]
    if y.numel() == 0:
        assert ks == [], ks
    else:
        fast = _is_fast(xd, x.shape, ch, U, hq, acc, frac)
        assert ks == ["fir1d_interp_kernel" if fast else "fir1d_interp_generic_kernel"], (U, len(hq), x.shape, ks)
    return y.cpu().numpy()


def _same(got, want, U, ch, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} outputs differ; the first at row {r}, output frame "
                             f"{k // ch} (input frame {k // ch // U}, phase {k // ch % U}), channel {k % ch}: "
                             f"{got[r, k]} != {want[r, k]}")


def _check(x, hq, U, frac, acc, stage, ch, what):
    rows, rowlen = x.shape
    want = _want(x, hq, U, frac, acc, stage, ch)
    assert want.shape == (rows, fir_hip.interp_out_width(rowlen // ch, U) * ch), what
    _same(_run(x, hq, U, frac, acc, stage, ch), want, U, ch, what)


# ---- 1. tile and row edges, fast kernel ---------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("U", [2, 3, 4, 5, 8, 15, 16])
def test_fast_kernel_tile_and_row_edges(U, cfg):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(1000 * U + len(cfg))
    T, G = _tile(cfg, U)
    shapes = [(1, T - 1), (1, T), (1, T + 1), (1, 2 * T + 3), (1, G * T - 1), (1, G * T + 1), (3, 8), (5, 1032),
              (2, T + 8)]
    shapes += [s for s in ((1, PASS - 1), (1, PASS + 1), (2, PASS + 8)) if s not in shapes]  # the edges of a pass
    xs = [_samples(rng, dtype, r, w, ch) for r, w in shapes]
    for L in sorted({1, 2, U - 1, U, U + 1, 9, 31, 64, 127, 128}):
        hq = rng.integers(-2000, 2001, L)
        for x in xs:
            _check(x, hq, U, 12, 32, stage, ch, (U, L, x.shape, cfg))
    # rows narrower than the window, ceil(L / U) frames
    x = _samples(rng, dtype, 4, 8, ch)
    _check(x, rng.integers(-2000, 2001, 128), U, 12, 32, stage, ch, (U, 128, "narrow", cfg))


# ---- 2. generic kernel branches -------------------------------------------------------------
def _generic_cases():
    c = []
    for U in (1, 17, 64, 1000):
        for L in (5, 129):
            c.append((f"U{U}_L{L}", dict(U=U, L=L, shape=(3, 67) if U == 1000 else (3, 1061))))
    for L in (129, 300):
        c.append((f"L{L}_U4", dict(U=4, L=L, cfg="u8_u8")))
        c.append((f"L{L}_U4_c16", dict(U=4, L=L, cfg="c16_i32")))
    c.append(("channels3", dict(U=4, L=9, ch=3)))
    c.append(("channels3_U1", dict(U=1, L=33, ch=3, shape=(3, 257))))
    c.append(("channels2_u8", dict(U=4, L=9, ch=2, cfg="u8_i32")))
    c.append(("acc40_u8", dict(U=2, L=5, acc=40, frac=33, cfg="u8_i32")))
    c.append(("acc48", dict(U=4, L=9, acc=48, frac=20)))
    c.append(("acc64", dict(U=3, L=31, acc=64, frac=12)))
    c.append(("acc33", dict(U=4, L=9, acc=33, frac=12)))
    c.append(("frac32", dict(U=4, L=9, acc=32, frac=32)))
    c.append(("x_off_2", dict(U=4, L=9, lead=2)))
    c.append(("x_off_8_i16", dict(U=4, L=9, lead=8)))
    c.append(("x_off_4_u8", dict(U=2, L=5, lead=4, cfg="u8_u8")))
    c.append(("x_off_2_complex", dict(U=8, L=64, lead=2, cfg="c16_i32")))
    c.append(("ragged_rows", dict(U=4, L=9, shape=(5, 1031))))
    c.append(("ragged_rows_u8", dict(U=2, L=5, shape=(5, 1031), cfg="u8_u8")))
    c.append(("tap_above_int16", dict(U=4, L=9, big_tap=32768)))
    c.append(("tap_below_int16", dict(U=4, L=9, big_tap=-32769)))
    c.append(("U_above_L_and_width", dict(U=700, L=9, shape=(6, 50))))
    return c


@pytest.mark.parametrize("name,case", _generic_cases(), ids=[n for n, _ in _generic_cases()])
def test_generic_kernel_branches(name, case):
    dtype, stage, ch = CONFIGS[case.get("cfg", "i16_i32")]
    ch = case.get("ch", ch)
    U, L = case["U"], case["L"]
    rng = np.random.default_rng(sum(map(ord, name)))  # a seed that does not change from run to run
    rows, width = case.get("shape", (3, 1061))
    x = _samples(rng, dtype, rows, width, ch)
    hq = rng.integers(-2000, 2001, L)
    if "big_tap" in case:
        hq[L // 2] = case["big_tap"]
    frac, acc = case.get("frac", 12), case.get("acc", 32)
    want = _want(x, hq, U, frac, acc, stage, ch)
    if "lead" in case:
        xd = guarded_input(torch.from_numpy(x), lead_bytes=case["lead"], device=DEV)
        assert xd.data_ptr() % 16 == case["lead"]
    else:
        xd = torch.from_numpy(x).to(DEV)
    got = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, U, frac, acc, stage, ch).cpu().numpy()
    _same(got, want, U, ch, name)


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
        _check(x, hq, 3, frac, acc, stage, 1, ("wide", frac, acc))


def test_up_1_equals_the_full_rate_entry():
    rng = np.random.default_rng(11)
    for cfg, (dtype, stage, ch) in CONFIGS.items():
        x = _samples(rng, dtype, 5, 1032, ch)
        xd = torch.from_numpy(x).to(DEV)
        for L in (5, 31, 129):
            hq = rng.integers(-2000, 2001, L)
            full = torch_ops.fir1d_fixed_rows_dev(xd, hq, 12, 32, stage, ch)
            got = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, 1, 12, 32, stage, ch)
            assert got.shape == full.shape and torch.equal(got, full), (cfg, L)


# ---- 3. arithmetic extremes, both kernels -----------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("U,L", [(2, 128), (3, 64), (8, 5), (17, 64), (4, 129)], ids=lambda v: str(v))
def test_arithmetic_extremes(U, L, cfg):
    """Taps at -32768 / 32767 against samples at the ends of their range: the 32-bit accumulator
    wraps many times over and v_dot2 must wrap, not saturate.  (17, 64) and (4, 129) run the
    generic kernel."""
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(U * 1000 + L)
    lo, hi = (0, 255) if dtype == np.uint8 else (-32768, 32767)
    rows, width = 2, _tile(cfg, U)[0] + 24
    x = np.where(rng.integers(0, 2, (rows, width * ch)) == 0, lo, hi).astype(dtype)
    x[0, : 64 * ch] = hi  # runs of one sign, so whole windows add up
    x[1, -64 * ch:] = lo
    xd = torch.from_numpy(x).to(DEV)
    xu = _stuff(x, U, ch)
    taps = [np.where(rng.integers(0, 2, L) == 0, -32768, 32767), np.full(L, 32767), np.full(L, -32768)]
    for hq in taps:
        for acc in (8, 16, 24, 32):
            for frac in (1, 12, 31):
                for st in (fir_hip.OUT_U8_SAT, fir_hip.OUT_I32):
                    want = c_oracle().fir1d_rows(xu, hq, frac, acc, st, channels=ch)
                    got = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, U, frac, acc, st, ch).cpu().numpy()
                    _same(got, want, U, ch, (U, L, cfg, int(hq[0]), acc, frac, st))


# ---- 4. guard bands -----------------------------------------------------------------------------
# shapes whose last tile is partial; x at leads on both sides of the fast path's alignment condition
# (16 bytes, u8: 8), y at every kind of lead: the fast kernel has no condition on y, its first and
# last 16-byte vector of a tile go out element by element
GUARDED = [
    # cfg, U, L, (rows, width), x_lead, y_lead, fast
    ("u8_u8", 2, 5, (3, 512 + 40), 8, 3, True),
    ("u8_i32", 5, 31, (1, 512 + 13), 0, 4, True),
    ("i16_u8", 16, 128, (2, 2048 + 72), 16, 1, True),
    ("i16_i32", 3, 64, (1, 1024 + 7), 0, 12, True),
    ("c16_i32", 16, 33, (3, 256 + 20), 32, 8, True),
    ("i16_i32", 4, 9, (8, 512 + 8), 48, 0, True),
    # generic: a misaligned x, and rows that are no multiple of 8 samples with a long filter
    ("i16_i32", 4, 9, (3, 1031), 2, 4, False),
    ("u8_u8", 17, 300, (5, 1031), 1, 5, False),
    ("u8_u8", 2, 5, (3, 552), 4, 3, False),
]


@pytest.mark.parametrize("cfg,U,L,shape,x_lead,y_lead,fast", GUARDED)
def test_guard_bands(cfg, U, L, shape, x_lead, y_lead, fast):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(U * 100 + L)
    x = _samples(rng, dtype, shape[0], shape[1], ch)
    hq = rng.integers(-2000, 2001, L)
    want = _want(x, hq, U, 12, 32, stage, ch)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    aligned = xd.data_ptr() % (8 if dtype == np.uint8 else 16) == 0
    rows_ok = shape[0] == 1 or (shape[1] * ch) % 8 == 0
    assert fast == (aligned and rows_ok and 2 <= U <= 16 and L <= 128)
    assert shape[1] % _tile(cfg, U)[0] != 0  # the last tile is partial
    yd, check = guarded_output((shape[0], shape[1] * U * ch), torch.uint8 if stage == fir_hip.OUT_U8_SAT else torch.int32,
                               lead_bytes=y_lead, device=DEV)
    assert yd.data_ptr() % 16 == y_lead
    out = torch_interp.fir1d_fixed_rows_interp_dev(xd, hq, U, 12, 32, stage, ch, out=yd)
    assert out is yd
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), want, U, ch, (cfg, U, L))
    check(f"{cfg} U={U}")


# ---- 5. one medium size per kernel family -----------------------------------------------------------
@pytest.mark.parametrize("cfg", ["i16_i32", "c16_i32"])
def test_medium_int16(cfg):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(22)
    x = _samples(rng, dtype, 1, 1 << 20, ch)
    _check(x, rng.integers(-3000, 3001, 33), 4, 12, 32, stage, ch, cfg)


def test_medium_u8_rows():
    rng = np.random.default_rng(23)
    x = _samples(rng, np.uint8, 1024, 4096, 1)
    _check(x, [-256, -1024, 6656, -1024, -256], 2, 12, 32, fir_hip.OUT_U8_SAT, 1, "u8 rows")


# ---- 6. graph capture -----------------------------------------------------------------------------
def test_fast_path_is_capturable():
    """The fast path allocates nothing and reads no device table: captured on one stream (a single
    linear chain, no parallel branches), replayed twice with x changed in place between replays."""
    rng = np.random.default_rng(6)
    U, L = 4, 33
    hq = torch_ops.Taps(rng.integers(-3000, 3001, L))
    shapes = {"i16_i32": (1, 3 * 512 + 40), "c16_i32": (2, 512 + 16), "u8_u8": (8, 4096)}
    xs = {k: torch.zeros((r, w * CONFIGS[k][2]), dtype=torch.uint8 if CONFIGS[k][0] == np.uint8 else torch.int16,
                         device=DEV) for k, (r, w) in shapes.items()}
    ys = {k: torch.empty((r, w * U * CONFIGS[k][2]),
                         dtype=torch.uint8 if CONFIGS[k][1] == fir_hip.OUT_U8_SAT else torch.int32, device=DEV)
          for k, (r, w) in shapes.items()}

    def step():
        for k in shapes:
            torch_interp.fir1d_fixed_rows_interp_dev(xs[k], hq, U, 12, 32, CONFIGS[k][1], CONFIGS[k][2], out=ys[k])

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
            want = _want(host[k], hq.h, U, 12, 32, CONFIGS[k][1], CONFIGS[k][2])
            _same(ys[k].cpu().numpy(), want, U, CONFIGS[k][2], (seed, k))


# ---- 7. empty problems, out= reuse, the host entry ---------------------------------------------------
def test_empty_problems_and_out_reuse():
    hq = [-256, -1024, 6656, -1024, -256]
    for shape, U, ch in (((0, 64), 4, 1), ((5, 0), 4, 1), ((5, 0), 1, 1), ((4, 0), 16, 2), ((0,), 2, 1), ((0, 6), 1000, 3)):
        x = torch.zeros(shape, dtype=torch.int16, device=DEV)
        y = torch_interp.fir1d_fixed_rows_interp_dev(x, hq, U, channels=ch)
        assert y.dtype == torch.int32 and y.numel() == 0
        assert tuple(y.shape) == tuple(shape[:-1]) + (shape[-1] * U,)
    rng = np.random.default_rng(7)
    out = torch.empty((3, 4128), dtype=torch.int32, device=DEV)
    for seed in (1, 2):  # the same out buffer, twice: nothing of the first call survives
        x = _samples(np.random.default_rng(seed), np.int16, 3, 1032, 1)
        got = torch_interp.fir1d_fixed_rows_interp_dev(torch.from_numpy(x).to(DEV), hq, 4, out=out)
        assert got is out
        _same(out.cpu().numpy(), _want(x, hq, 4, 12, 32, fir_hip.OUT_I32, 1), 4, 1, ("reuse", seed))
    x = torch.from_numpy(_samples(rng, np.int16, 3, 1032, 1)).to(DEV)
    for bad in (torch.empty((3, 4128), dtype=torch.uint8, device=DEV), torch.empty((3, 1032), dtype=torch.int32, device=DEV),
                torch.empty((3, 4127), dtype=torch.int32, device=DEV), torch.empty((3, 4128), dtype=torch.int32)):
        with pytest.raises(fir_hip.FirHipError, match="out must"):
            torch_interp.fir1d_fixed_rows_interp_dev(x, hq, 4, out=bad)
    for U in (0, -4):
        with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):
            torch_interp.fir1d_fixed_rows_interp_dev(x, hq, U)
    # the host entry, through the same kernels: the fast one, and the generic one
    xh = _samples(rng, np.uint8, 7, 4096, 1)
    _same(fir_hip.fir1d_fixed_rows_interp(xh, hq, 8), _want(xh, hq, 8, 12, 32, fir_hip.OUT_U8_SAT, 1), 8, 1, "host fast")
    xc = _samples(rng, np.int16, 3, 515, 2)
    got = fir_hip.fir1d_fixed_rows_interp(xc, hq, 17, 14, 40, fir_hip.OUT_I32, channels=2)
    _same(got, _want(xc, hq, 17, 14, 40, fir_hip.OUT_I32, 2), 17, 2, "host generic")
    y = np.empty((7, 4096 * 3), np.uint8)
    assert fir_hip.fir1d_fixed_rows_interp(xh, hq, 3, out=y) is y
    _same(y, _want(xh, hq, 3, 12, 32, fir_hip.OUT_U8_SAT, 1), 3, 1, "host out=")
    assert fir_hip.fir1d_fixed_rows_interp(np.zeros((4, 0), np.uint8), hq, 5).shape == (4, 0)


# ---- 8. the argument contract on device tensors -------------------------------------------------------
@pytest.mark.parametrize("case", ic.CASES, ids=[c.id for c in ic.CASES])
def test_contract_case_on_device_tensors(case, monkeypatch):
    """tests/torch_interp_cases.py on real cuda:0 tensors, still against the stub library: nothing
    is launched, a refused case never reaches the real library."""
    ic.run(case, ic.Maker(standin=False), torch_interp, monkeypatch)
