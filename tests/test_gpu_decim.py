"""GPU: the decimating 1-D FIR (fir_decim_rows_dev through torch_ops.fir1d_fixed_rows_decim_dev).

The reference for every value is the committed C oracle at full rate, then a NumPy slice:

    c_oracle().fir1d_rows(x, hq, frac, acc, stage, channels=ch).reshape(rows, width, ch)[:, phase::D]

so every comparison is np.array_equal, no tolerance.  T below is the number of output frames one
workgroup of the fast kernel owns (kDecT, stated in the header comment of csrc/fir1d_decim.hip):
the shapes are built around it so that tiles end exactly at, one short of and one past a row's
end.  The fast kernel runs when decim_path_ok holds (2 <= D <= 16, L <= 128 taps within int16,
acc_bits <= 32, frac_bits <= 31, u8 x 1 channel or int16 x 1 | 2, x 16-byte aligned (u8: 8), one
row or rows of a multiple of 8 samples); every other call takes the generic kernel.  No test here
provokes a fault: all buffers are in bounds, the guarded cases sit inside one allocation.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output
from rate_property_cases import decim_want as _want  # the reference above, stated once for the grid and the property tests

DEV = torch.device("cuda:0")
T = 512  # kDecT: output frames per workgroup of fir1d_decim_kernel (csrc/fir1d_decim.hip, header comment)

# name -> (sample dtype, out_stage, channels)
CONFIGS = {
    "u8_u8": (np.uint8, fir_hip.OUT_U8_SAT, 1),
    "u8_i32": (np.uint8, fir_hip.OUT_I32, 1),
    "i16_u8": (np.int16, fir_hip.OUT_U8_SAT, 1),
    "i16_i32": (np.int16, fir_hip.OUT_I32, 1),
    "c16_i32": (np.int16, fir_hip.OUT_I32, 2),
}


def _samples(rng, dtype, rows, width, ch):
    lo, hi = (0, 256) if dtype == np.uint8 else (-32768, 32768)
    return rng.integers(lo, hi, (rows, width * ch), dtype=dtype)


def _is_fast(xd, shape, ch, D, hq, acc, frac):
    """decim_path_ok, from the documented conditions (the module docstring, fir_launch.h)."""
    u8 = xd.dtype == torch.uint8
    h = [int(v) for v in np.asarray(hq, dtype=object).reshape(-1)]
    return (2 <= D <= 16 and len(h) <= 128 and min(h) >= -32768 and max(h) <= 32767 and acc <= 32 and frac <= 31
            and (ch == 1 or (ch == 2 and not u8)) and xd.data_ptr() % (8 if u8 else 16) == 0
            and (shape[0] == 1 or shape[1] % 8 == 0))


def _run(x, hq, D, phase, frac, acc, stage, ch, **kw):
    """The device entry, its launch log held against _is_fast (an empty output launches nothing)."""
    xd = torch.from_numpy(x).to(DEV)
    with fir_hip.launch_log() as log:
        y = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq, D, phase, frac, acc, stage, ch, **kw)
    ks = [l.kernel for l in log]
    if y.numel() == 0:
        assert ks == [], ks
    else:
        fast = _is_fast(xd, x.shape, ch, D, hq, acc, frac)
        assert ks == ["fir1d_decim_kernel" if fast else "fir1d_decim_generic_kernel"], (D, len(hq), x.shape, ks)
    return y.cpu().numpy()


def _check(x, hq, D, phase, frac, acc, stage, ch, what):
    rows, rowlen = x.shape
    want = _want(x, hq, D, phase, frac, acc, stage, ch)
    got = _run(x, hq, D, phase, frac, acc, stage, ch)
    assert got.shape == (rows, want.shape[1] * ch), what
    assert want.shape[1] == fir_hip.decim_out_width(rowlen // ch, D, phase), what
    got = got.reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, m, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} outputs differ; the first at row {r}, frame {m}, "
                             f"channel {c}: {got[r, m, c]} != {want[r, m, c]}")


# ---- 1. tile and row edges, fast kernel ---------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("D", [2, 3, 4, 5, 8, 15, 16])
def test_fast_kernel_tile_and_row_edges(D, cfg):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(1000 * D + len(cfg))
    G = max(1, 16 // D)  # tiles one workgroup owns (same header comment): its edge is at G * T outputs
    for phase in sorted({0, 1, D - 1}):
        shapes = [(1, D * T - 1), (1, D * T), (1, D * T + 1), (1, D * T + phase + 1), (1, 2 * D * T + 3),
                  (3, 8), (5, 1032), (2, D * T + 8)]
        if G > 1:
            shapes += [(1, G * D * T - 1), (1, G * D * T + phase + 1), (2, G * D * T + 8)]
        xs = [_samples(rng, dtype, r, w, ch) for r, w in shapes]
        for L in (1, 2, 5, 9, 10, 31, 64, 127, 128):
            hq = rng.integers(-2000, 2001, L)
            for x in xs:
                _check(x, hq, D, phase, 12, 32, stage, ch, (D, phase, L, x.shape, cfg))
        # a row narrower than the filter
        x = _samples(rng, dtype, 4, 8, ch)
        _check(x, rng.integers(-2000, 2001, 31), D, phase, 12, 32, stage, ch, (D, phase, 31, "narrow", cfg))


# ---- 2. generic kernel branches -------------------------------------------------------------
def _generic_cases():
    c = []
    for D in (1, 17, 64, 1000):
        for L in (5, 129):
            c.append((f"D{D}_L{L}", dict(D=D, L=L)))
    for L in (129, 300):
        c.append((f"L{L}_D4", dict(D=4, L=L, cfg="u8_u8")))
        c.append((f"L{L}_D16_c16", dict(D=16, L=L, cfg="c16_i32")))
    c.append(("channels3", dict(D=4, L=9, ch=3)))
    c.append(("channels3_D1", dict(D=1, L=33, ch=3, shape=(3, 257))))
    c.append(("acc48", dict(D=4, L=9, acc=48, frac=20)))
    c.append(("acc64", dict(D=3, L=31, acc=64, frac=12)))
    c.append(("acc40_u8", dict(D=2, L=5, acc=40, frac=33, cfg="u8_i32")))
    c.append(("x_off_2", dict(D=4, L=9, lead=2)))
    c.append(("x_off_2_complex", dict(D=8, L=64, lead=2, cfg="c16_i32")))
    c.append(("ragged_rows", dict(D=4, L=9, shape=(5, 1031))))
    c.append(("ragged_rows_u8", dict(D=2, L=5, shape=(5, 1031), cfg="u8_u8")))
    c.append(("tap_above_int16", dict(D=4, L=9, big_tap=32768)))
    c.append(("tap_below_int16", dict(D=4, L=9, big_tap=-32769)))
    c.append(("D_above_width", dict(D=700, L=9, shape=(6, 500), phases=(0, 250, 499, 699))))
    return c


@pytest.mark.parametrize("name,case", _generic_cases(), ids=[n for n, _ in _generic_cases()])
def test_generic_kernel_branches(name, case):
    dtype, stage, ch = CONFIGS[case.get("cfg", "i16_i32")]
    ch = case.get("ch", ch)
    D, L = case["D"], case["L"]
    rng = np.random.default_rng(sum(map(ord, name)))  # a seed that does not change from run to run
    rows, width = case.get("shape", (3, 2 * T + 37))
    x = _samples(rng, dtype, rows, width, ch)
    hq = rng.integers(-2000, 2001, L)
    if "big_tap" in case:
        hq[L // 2] = case["big_tap"]
    frac, acc = case.get("frac", 12), case.get("acc", 32)
    for phase in case.get("phases", sorted({0, 1 % D, D - 1})):
        want = _want(x, hq, D, phase, frac, acc, stage, ch)
        if "lead" in case:
            xd = guarded_input(torch.from_numpy(x), lead_bytes=case["lead"], device=DEV)
            assert xd.data_ptr() % 16 == case["lead"]
        else:
            xd = torch.from_numpy(x).to(DEV)
        got = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq, D, phase, frac, acc, stage, ch).cpu().numpy()
        assert np.array_equal(got.reshape(want.shape), want), (name, phase)
        if D > width:
            assert want.shape[1] == (1 if phase < width else 0)


def test_generic_kernel_wide_sums():
    """needs_wide: 2^17 + 9 taps of +-(2^31 - 1) make sum|h| * 32768 pass 2^63, so the generic
    kernel sums in 128 bits; the samples are small (|x| <= 100), so every true sum stays far
    below 2^63 and the C oracle's 64-bit sums are exact."""
    rng = np.random.default_rng(63)
    L = (1 << 17) + 9
    hq = np.where(rng.integers(0, 2, L) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert int(np.abs(hq).sum()) * 32768 >= 1 << 63
    x = rng.integers(-100, 101, (2, 1500), dtype=np.int16)
    for frac, acc, stage in ((30, 64, fir_hip.OUT_I32), (40, 80, fir_hip.OUT_U8_SAT)):
        _check(x, hq, 3, 2, frac, acc, stage, 1, ("wide", frac, acc))


def test_decim_1_equals_the_full_rate_entry():
    rng = np.random.default_rng(11)
    for cfg, (dtype, stage, ch) in CONFIGS.items():
        x = _samples(rng, dtype, 5, 1032, ch)
        xd = torch.from_numpy(x).to(DEV)
        for L in (5, 31, 129):
            hq = rng.integers(-2000, 2001, L)
            full = torch_ops.fir1d_fixed_rows_dev(xd, hq, 12, 32, stage, ch)
            got = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq, 1, 0, 12, 32, stage, ch)
            assert got.shape == full.shape and torch.equal(got, full), (cfg, L)


# ---- 3. arithmetic extremes, both kernels -----------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("D,L", [(2, 64), (3, 128), (8, 5), (17, 64), (4, 129)], ids=lambda v: str(v))
def test_arithmetic_extremes(D, L, cfg):
    """Taps at -32768 / 32767 against samples at the ends of their range: the 32-bit accumulator
    wraps many times over and v_dot2 must wrap, not saturate.  (17, 64) and (4, 129) run the
    generic kernel."""
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(D * 1000 + L)
    lo, hi = (0, 255) if dtype == np.uint8 else (-32768, 32767)
    rows, width = 2, D * T + 24
    x = np.where(rng.integers(0, 2, (rows, width * ch)) == 0, lo, hi).astype(dtype)
    x[0, : 64 * ch] = hi  # runs of one sign, so whole windows add up
    x[1, -64 * ch:] = lo
    taps = [np.where(rng.integers(0, 2, L) == 0, -32768, 32767), np.full(L, 32767), np.full(L, -32768)]
    for hq in taps:
        for acc in (8, 16, 24, 32):
            for frac in (1, 12, 31):
                for st in (fir_hip.OUT_U8_SAT, fir_hip.OUT_I32):
                    _check(x, hq, D, D - 1, frac, acc, st, ch, (D, L, cfg, int(hq[0]), acc, frac, st))


# ---- 4. guard bands -----------------------------------------------------------------------------
# shapes whose last tile is partial and whose rows end inside a 16-byte vector of the output
GUARDED = [
    # cfg, D, phase, L, (rows, width), x_lead, y_lead
    ("u8_u8", 2, 1, 5, (3, 2 * T + 40), 8, 3),
    ("u8_i32", 5, 4, 31, (1, 5 * T + 13), 0, 4),
    ("i16_u8", 16, 7, 128, (2, 16 * T + 72), 16, 1),
    ("i16_i32", 3, 0, 64, (1, 3 * T + 7), 0, 12),
    ("c16_i32", 8, 3, 33, (3, 8 * T + 20), 32, 8),
    # generic: a misaligned x, and rows that are no multiple of 8 samples with a long filter
    ("i16_i32", 4, 1, 9, (3, 1031), 2, 4),
    ("u8_u8", 17, 16, 300, (5, 1031), 1, 5),
]


@pytest.mark.parametrize("cfg,D,phase,L,shape,x_lead,y_lead", GUARDED)
def test_guard_bands(cfg, D, phase, L, shape, x_lead, y_lead):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(D * 100 + L)
    x = _samples(rng, dtype, shape[0], shape[1], ch)
    hq = rng.integers(-2000, 2001, L)
    want = _want(x, hq, D, phase, 12, 32, stage, ch)
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    ow = fir_hip.decim_out_width(shape[1], D, phase)
    assert (ow * ch * want.itemsize) % 16 != 0 or shape[0] == 1  # rows end inside a 16-byte vector
    assert ow % T != 0  # the last tile is partial
    yd, check = guarded_output((shape[0], ow * ch), torch.uint8 if stage == fir_hip.OUT_U8_SAT else torch.int32,
                               lead_bytes=y_lead, device=DEV)
    out = torch_ops.fir1d_fixed_rows_decim_dev(xd, hq, D, phase, 12, 32, stage, ch, out=yd)
    assert out is yd
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy().reshape(want.shape), want)
    check(f"{cfg} D={D}")


# ---- 5. one medium size ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["i16_i32", "c16_i32"])
def test_medium_int16(cfg):
    dtype, stage, ch = CONFIGS[cfg]
    rng = np.random.default_rng(22)
    x = _samples(rng, dtype, 1, 1 << 22, ch)
    _check(x, rng.integers(-3000, 3001, 33), 4, 1, 12, 32, stage, ch, cfg)


def test_medium_u8_rows():
    rng = np.random.default_rng(23)
    x = _samples(rng, np.uint8, 1024, 4096, 1)
    _check(x, [-256, -1024, 6656, -1024, -256], 2, 1, 12, 32, fir_hip.OUT_U8_SAT, 1, "u8 rows")


# ---- 6. graph capture -----------------------------------------------------------------------------
def test_fast_path_is_capturable():
    """The fast path allocates nothing and reads no device table: captured on one stream (a single
    linear chain, no parallel branches), replayed twice with x changed in place between replays."""
    rng = np.random.default_rng(6)
    D, phase, L = 4, 1, 33
    hq = torch_ops.Taps(rng.integers(-3000, 3001, L))
    shapes = {"i16_i32": (1, 3 * D * T + 40), "c16_i32": (2, D * T + 16), "u8_u8": (8, 4096)}
    xs = {k: torch.zeros((r, w * CONFIGS[k][2]), dtype=torch.uint8 if CONFIGS[k][0] == np.uint8 else torch.int16,
                         device=DEV) for k, (r, w) in shapes.items()}
    ys = {k: torch.empty((r, fir_hip.decim_out_width(w, D, phase) * CONFIGS[k][2]),
                         dtype=torch.uint8 if CONFIGS[k][1] == fir_hip.OUT_U8_SAT else torch.int32, device=DEV)
          for k, (r, w) in shapes.items()}

    def step():
        for k in shapes:
            torch_ops.fir1d_fixed_rows_decim_dev(xs[k], hq, D, phase, 12, 32, CONFIGS[k][1], CONFIGS[k][2], out=ys[k])

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
            want = _want(host[k], hq.h, D, phase, 12, 32, CONFIGS[k][1], CONFIGS[k][2])
            assert np.array_equal(ys[k].cpu().numpy().reshape(want.shape), want), (seed, k)


# ---- 7. empty problems and out= reuse ---------------------------------------------------------------
def test_empty_problems_and_out_reuse():
    hq = [-256, -1024, 6656, -1024, -256]
    for shape, D, phase, ch in (((0, 64), 4, 1, 1), ((5, 0), 4, 1, 1), ((5, 3), 8, 3, 1), ((5, 3), 8, 7, 1),
                                ((4, 6), 16, 3, 2), ((0,), 2, 0, 1)):
        x = torch.zeros(shape, dtype=torch.int16, device=DEV)
        y = torch_ops.fir1d_fixed_rows_decim_dev(x, hq, D, phase, channels=ch)
        assert y.dtype == torch.int32 and y.numel() == 0
        assert tuple(y.shape) == tuple(shape[:-1]) + (fir_hip.decim_out_width(shape[-1] // ch, D, phase) * ch,)
    rng = np.random.default_rng(7)
    out = torch.empty((3, 258), dtype=torch.int32, device=DEV)
    for seed in (1, 2):  # the same out buffer, twice: nothing of the first call survives
        x = _samples(np.random.default_rng(seed), np.int16, 3, 1032, 1)
        got = torch_ops.fir1d_fixed_rows_decim_dev(torch.from_numpy(x).to(DEV), hq, 4, 1, out=out)
        assert got is out
        assert np.array_equal(out.cpu().numpy().reshape(3, 258, 1), _want(x, hq, 4, 1, 12, 32, fir_hip.OUT_I32, 1))
    x = torch.from_numpy(_samples(rng, np.int16, 3, 1032, 1)).to(DEV)
    for bad in (torch.empty((3, 258), dtype=torch.uint8, device=DEV), torch.empty((3, 1032), dtype=torch.int32, device=DEV),
                torch.empty((3, 259), dtype=torch.int32, device=DEV), torch.empty((3, 258), dtype=torch.int32)):
        with pytest.raises(fir_hip.FirHipError):
            torch_ops.fir1d_fixed_rows_decim_dev(x, hq, 4, 1, out=bad)
    for D, phase in ((0, 0), (4, 4), (4, -1)):
        with pytest.raises(fir_hip.FirHipError, match="decim|phase"):
            torch_ops.fir1d_fixed_rows_decim_dev(x, hq, D, phase)
    # the host entry, through the same kernels
    xh = _samples(rng, np.uint8, 7, 4096, 1)
    got = fir_hip.fir1d_fixed_rows_decim(xh, hq, 8, 5)
    assert np.array_equal(got.reshape(7, 512, 1), _want(xh, hq, 8, 5, 12, 32, fir_hip.OUT_U8_SAT, 1))
