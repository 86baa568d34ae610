"""The case table and helpers of tests/test_gpu_big_index.py -- a test helper, not a test module.

The 1-D kernels at sizes where a sample index passes 2^31 or 2^32, or a byte offset does, on the
input or on the output side.  Signals of 2-4 x 10^9 samples cannot pass through the CPU oracle in
a test's time, so the input is PERIODIC with a prime period:

* one row: ``P`` frames of uniform random samples, tiled into a row of ``n`` frames.  Away from
  the two row ends the output of every family then repeats every ``T = P * U`` output frames
  (U = 1 where the family does not interpolate; a shift of T output frames is a shift of T * D / U
  = P * D input frames, a whole number of periods, for any D, phase, tap count and channel count);
* many rows: ``Q`` distinct random rows, row r of x being row r % Q of them, so output row r
  equals output row r % Q.

No power of two is a multiple of P, of Q or of Q * rowlen, so a read or a write displaced by a
power-of-two number of elements or bytes never lands on an equal value: ``verify`` compares every
interior period with period 1 (every row with row r % Q) on the device, which shows a displaced
tile and, through the 0x5A sentinel the output was filled with, its untouched destination; then it
copies back periods 0-1, the last two periods and the ragged tail (rows 0 .. Q-1 and the last Q
rows) and compares them bit for bit with the references the other GPU tests use, run on the
matching slice of x with a lead-in that is thrown away, which shows an error common to every
period.

Everything here works on tensors of any device: tests/test_big_index_cases.py runs the same table
(``table(SMALL)``: every threshold 2^12, a short period) and the same ``verify`` on the CPU, the
oracle standing in for the device, and holds ``verify`` against planted displacements.

``dispatch_kernel`` restates the dispatch conditions of csrc (decim_path_ok, interp_path_ok,
resample_path_ok, cplx_path_ok here; reg_path_ok, mfma_path_ok and the k-step count of
launch_mfma_t, lds_path_ok and the register test of launch_fir1d_ideal in
tests/fullrate_property_cases.py, which states them once); ``Case.kernel`` is the kernel each
large case was built for, and the two must agree before a case runs.

The four complex-rate extension libraries (families ``cdecim``, ``cinterp``, ``cresample`` and
``cstream``: complex int16 frames, one dword in and an int32 pair out) write nothing to the launch
log; their ``Case.kernel`` is the (route, bucket) of the library's own record as a string such as
``"cdecim:FAST/12"``, and ``dispatch_kernel`` gives the ``predicted_route`` of the family's
``*_cases.py`` helper in that form.  A ``cstream`` case is one block behind a hostile history
(``make_hist``; row r has history r % Q, so the rows still repeat with Q): its y is checked like
every other family's (the filter is causal, so from period 1 on the output has period P), and
``verify`` holds hist_out against the last taps - 1 frames of every row of x.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable

import numpy as np
import torch

import cdecim_cases
import cinterp_cases
import cplx_ref
import cresample_cases
import cstream_cases
import fir_hip
from fir_hip import cdecim, cinterp, cresample, cstream
from oracle import c_oracle
from fullrate_property_cases import Case as FullRateCase
from fullrate_property_cases import _mfma_ksteps, bank_fused, ideal_kernel, rows_kernel  # noqa: F401  (_mfma_ksteps: re-exported)
from rate_property_cases import decim_want, interp_want, resample_want

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
FRAC, ACC = 12, 32
SENTINEL = 0x5A
GIB = 1 << 30
CAP_BYTES = 24 * GIB          # x + y + compare temporaries of one case
TEMP_BYTES = 1 * GIB          # the compare temporaries' share of it
CHUNK = 1 << 28               # elements compared at once: a bool and a uint8 temporary of 256 MiB each
FILL = 1 << 26                # elements of the tiled block x is filled from
CEXT = {"cdecim": (cdecim, cdecim_cases), "cinterp": (cinterp, cinterp_cases), "cresample": (cresample, cresample_cases),
        "cstream": (cstream, cstream_cases)}  # family: (the library's ctypes module, its test helper)
ROUTES = ("NONE", "FAST", "GENERIC32", "GENERIC64", "GENERIC128")  # FIR_C*_NONE .. _GENERIC128


@dataclass(frozen=True)
class Scale:
    """thr(e): the threshold that stands for 2^e; P, Q: the two prime periods; width: the row
    length of the many-rows cases."""
    thr: Callable[[int], int]
    P: int
    Q: int
    width: int


FULL = Scale(lambda e: 1 << e, 100_003, 1009, 4096)
SMALL = Scale(lambda e: 1 << 12, 101, 13, 64)  # the CPU self-test: 2^12 for every threshold


@dataclass(frozen=True)
class Case:
    """One call.  width: input frames per row.  x_off: elements x starts past a 16-byte boundary.
    crosses: (side, unit, exponent) claims, e.g. ("out", "byte", 33): the output's bytes pass
    thr(33); units are elem, byte and frame (ch elements), sides in, out, "stuffed" (the resampler's
    zero-stuffed index m * D + phase, which reaches width * U) and "hist" (a stream's rows * H history
    frames).  kernel: the kernel the case was built for (None for a twin: whatever dispatch_kernel
    says)."""
    name: str
    family: str          # fixed | bank | ideal | decim | interp | resample | cplx | cdecim | cinterp | cresample | cstream
    dtype: str           # u8 | i16
    stage: int | None    # U8 | I32; None: the float64 ideal model
    ch: int
    taps: int
    width: int
    rows: int = 1
    up: int = 1
    decim: int = 1
    phase: int = 0
    filters: int = 1
    x_off: int = 0
    kernel: str | None = None
    crosses: tuple = ()
    P: int = FULL.P
    Q: int = FULL.Q

    # ---- sizes ---------------------------------------------------------------------------------
    @property
    def in_itemsize(self) -> int:
        return 1 if self.dtype == "u8" else 2

    @property
    def out_itemsize(self) -> int:
        return 8 if self.stage is None else (4 if self.stage == I32 else 1)

    @property
    def out_width(self) -> int:
        """Output frames per row, by the library's own host functions."""
        if self.family == "decim":
            return fir_hip.decim_out_width(self.width, self.decim, self.phase)
        if self.family == "interp":
            return fir_hip.interp_out_width(self.width, self.up)
        if self.family == "resample":
            return fir_hip.resample_out_width(self.width, self.up, self.decim, self.phase)
        if self.family in ("cdecim", "cstream"):
            return CEXT[self.family][0].out_width(self.width, self.decim, self.phase)
        if self.family == "cinterp":
            return cinterp.out_width(self.width, self.up)
        if self.family == "cresample":
            return cresample.out_width(self.width, self.up, self.decim, self.phase)
        return self.width

    @property
    def in_elems(self) -> int:
        return self.rows * self.width * self.ch

    @property
    def out_elems(self) -> int:
        return self.filters * self.rows * self.out_width * self.ch

    @property
    def hist_frames(self) -> int:
        """H: the frames of history a stream's block reads and writes per row (0: not a stream)."""
        return self.taps - 1 if self.family == "cstream" else 0

    def size(self, side: str, unit: str) -> int:
        n = {"in": self.in_elems, "out": self.out_elems, "stuffed": self.in_elems * self.up,
             "hist": self.rows * self.hist_frames * self.ch}[side]
        if unit == "frame":
            return n // self.ch
        return n * (1 if unit == "elem" else (self.out_itemsize if side == "out" else self.in_itemsize))

    @property
    def footprint(self) -> int:
        """Device bytes of the case: x (with the slack an offset x is cut from), y, the temporaries;
        a stream's two histories, hist_out inside its guards (tests/guarded.py: 64 KiB and two rows
        a side, rounded up: 1 MiB covers them)."""
        hist = 2 * self.size("hist", "byte") + (1 << 20) if self.hist_frames else 0
        return (self.in_elems + 16) * self.in_itemsize + self.out_elems * self.out_itemsize + hist + TEMP_BYTES

    @property
    def period(self) -> int:
        """T: output frames after which a single row's output repeats."""
        return self.P * self.up

    @property
    def torch_in(self):
        return torch.uint8 if self.dtype == "u8" else torch.int16

    @property
    def torch_out(self):
        return torch.float64 if self.stage is None else (torch.int32 if self.stage == I32 else torch.uint8)

    @property
    def np_in(self):
        return np.uint8 if self.dtype == "u8" else np.int16

    @property
    def seed(self) -> int:
        return sum(map(ord, self.name.removeprefix("twin_")))  # a twin has its case's samples and taps


# ---- taps ------------------------------------------------------------------------------------------
def taps_of(c: Case):
    """The case's taps from its seed.  Real fixed taps: L ints whose sum is about U * 2^FRAC, so a
    u8 stage spreads over its range instead of saturating (a displaced tile must not meet a row of
    255s); bank: filters x L; ideal: L doubles; cplx and the complex-rate families: L (hr, hi) pairs."""
    rng = np.random.default_rng(c.seed)
    if c.family == "ideal":
        return rng.uniform(-1.0, 1.0, c.taps)
    if c.family == "cplx" or c.family in CEXT:
        return rng.integers(-2000, 2001, (c.taps, 2))
    h = rng.integers(50, 1200, (c.filters, c.taps)).astype(np.float64)
    h[:, 1::3] *= -0.25  # some negative taps; the sum stays well above zero
    h = np.rint(h * (c.up << FRAC) / h.sum(axis=1, keepdims=True)).astype(np.int64)
    assert np.abs(h).max() <= 32639  # int16 taps the matrix-core split can hold
    return h if c.family == "bank" else h[0]


# ---- the case table --------------------------------------------------------------------------------
def table(s: Scale = FULL) -> list[Case]:
    """Every large case, each followed by its twin at offset 0 (2 P frames, or 2 Q rows)."""
    P, Q, W, thr = s.P, s.Q, s.width, s.thr
    pad = 3 * P + 77               # a ragged partial period and a ragged last tile
    pad8 = (pad + 7) // 8 * 8      # ... for the kernels that need a row of whole 8-sample vectors
    assert pad8 % 1024 != 0 and pad % 8 != 0

    def up_to(n, m):
        return -(-n // m)

    big: list[Case] = []

    def add(name, family, dtype, stage, ch, taps, width, **kw):
        big.append(Case(name, family, dtype, stage, ch, taps, width, P=P, Q=Q, **kw))

    # full-rate fixed, one row
    add("fixed_u8_reg", "fixed", "u8", U8, 1, 5, thr(32) + pad, kernel="fir1d_reg_kernel",
        crosses=(("in", "elem", 32), ("out", "elem", 32)))
    add("fixed_i16_reg", "fixed", "i16", I32, 1, 5, thr(31) + pad, kernel="fir1d_reg_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "elem", 31), ("out", "byte", 33)))
    add("fixed_c16_reg", "fixed", "i16", I32, 2, 3, thr(30) + pad, kernel="fir1d_reg_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "elem", 31), ("out", "byte", 33)))
    add("fixed_u8_mfma16", "fixed", "u8", U8, 1, 16, thr(32) + pad8, kernel="fir1d_mfma_step_kernel",
        crosses=(("in", "elem", 32), ("out", "elem", 32)))
    add("fixed_i16_lds16", "fixed", "i16", I32, 1, 16, thr(31) + pad, kernel="fir1d_lds_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))
    add("fixed_i16_mfma48", "fixed", "i16", I32, 1, 48, thr(31) + pad8, kernel="fir1d_mfma_step_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))
    add("fixed_u8_run66", "fixed", "u8", U8, 1, 66, thr(32) + pad8, kernel="fir1d_mfma_run_kernel",
        crosses=(("in", "elem", 32), ("out", "elem", 32)))
    # 65 taps are three k-steps, the step kernel's last length (launch_mfma_t); the chunked kernel
    # starts at 66, so the chunked case has 66 and the 65-tap one stays as the step kernel's edge
    add("fixed_i16_step65", "fixed", "i16", I32, 1, 65, thr(31) + pad8, kernel="fir1d_mfma_step_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))
    add("fixed_i16_long66", "fixed", "i16", I32, 1, 66, thr(31) + pad8, kernel="fir1d_mfma_long_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))
    add("fixed_u8_generic", "fixed", "u8", U8, 1, 5, thr(32) + pad, x_off=1, kernel="fir1d_generic_kernel",
        crosses=(("in", "elem", 32), ("out", "elem", 32)))

    # full-rate fixed, many rows of W u8 samples, 5 taps
    add("rows_u8_reg_last", "fixed", "u8", U8, 1, 5, W, rows=thr(32) // W - 1, kernel="fir1d_reg_kernel",
        crosses=(("in", "elem", 31), ("out", "elem", 31)))           # total = 2^32 - W: the last size on it
    add("rows_u8_reg_first_off", "fixed", "u8", U8, 1, 5, W, rows=thr(32) // W, kernel="fir1d_lds_kernel",
        crosses=(("in", "elem", 31), ("out", "elem", 31)))           # total = 2^32: the first size off it
    add("bank4_u8_rows", "bank", "u8", U8, 1, 5, W, rows=thr(31) // W + 3, filters=4, kernel="fir1d_reg_kernel",
        crosses=(("in", "elem", 31), ("out", "elem", 33)))

    # float64 ideal
    add("ideal_one_row", "ideal", "u8", None, 1, 5, thr(31) + pad, kernel="fir1d_ideal_reg_kernel",
        crosses=(("in", "elem", 31), ("out", "elem", 31), ("out", "byte", 32), ("out", "byte", 34)))
    add("ideal_rows", "ideal", "u8", None, 1, 5, W, rows=thr(31) // W + 3, kernel="fir1d_ideal_reg_kernel",
        crosses=(("in", "elem", 31), ("out", "byte", 34)))           # (uint32_t)g0 % rowlen32 with the top bit set

    # the rate-changing and complex-tap families: the fast kernel, then the generic one (x one element off)
    def both(name, family, kernel, *a, **kw):
        add(name + "_fast", family, *a, kernel=kernel + "_kernel", **kw)
        add(name + "_generic", family, *a, kernel=kernel + "_generic_kernel", x_off=1, **kw)

    both("decim_u8_D2", "decim", "fir1d_decim", "u8", U8, 1, 5, thr(32) + pad, decim=2, phase=1,
         crosses=(("in", "elem", 32), ("out", "elem", 31)))
    both("decim_i16_D2", "decim", "fir1d_decim", "i16", I32, 1, 9, thr(32) + pad, decim=2, phase=0,
         crosses=(("in", "elem", 32), ("in", "byte", 33), ("out", "elem", 31), ("out", "byte", 33)))
    both("decim_c16_D3", "decim", "fir1d_decim", "i16", I32, 2, 9, thr(31) + pad, decim=3, phase=2,
         crosses=(("in", "elem", 32), ("in", "byte", 33), ("out", "byte", 32)))
    both("interp_u8_U16", "interp", "fir1d_interp", "u8", I32, 1, 16, thr(27) + pad, up=16,
         crosses=(("out", "elem", 31), ("out", "byte", 33)))
    both("interp_i16_U2", "interp", "fir1d_interp", "i16", I32, 1, 9, thr(30) + pad, up=2,
         crosses=(("in", "byte", 31), ("out", "elem", 31), ("out", "byte", 33)))
    both("resample_i16_3_2", "resample", "fir1d_resample", "i16", I32, 1, 72, up_to(2 * thr(31), 3) + pad, up=3,
         decim=2, phase=1, crosses=(("out", "elem", 31), ("out", "byte", 33), ("in", "byte", 31)))
    both("resample_u8_2_3", "resample", "fir1d_resample", "u8", U8, 1, 9, thr(32) + pad, up=2, decim=3, phase=2,
         crosses=(("in", "elem", 32), ("out", "elem", 31)))
    add("cplx_5_fast", "cplx", "i16", I32, 2, 5, thr(30) + pad, kernel="fir1d_cplx_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))
    add("cplx_65_generic", "cplx", "i16", I32, 2, 65, thr(30) + pad, kernel="fir1d_cplx_generic32_kernel",
        crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 33)))

    # the complex-rate extension libraries: complex int16 frames (one dword in, an int32 pair out).
    # fast: x at a 16-byte boundary; generic32: x 4 bytes off it; generic64: x 2 bytes off it.
    def cext(name, family, route, taps, width, *, x_off=0, **kw):
        add(name, family, "i16", I32, 2, taps, width, kernel=f"{family}:{route}", x_off=x_off, **kw)

    def fast_and_g32(name, family, bucket, taps, width, **kw):
        cext(name + "_fast", family, f"FAST/{bucket}", taps, width, **kw)
        cext(name + "_generic32", family, "GENERIC32/0", taps, width, x_off=2, **kw)

    many = thr(31) // W + 3        # rows of W frames whose r * width passes thr(31) frames
    d2 = (("in", "frame", 31), ("in", "byte", 33), ("out", "elem", 31), ("out", "byte", 33))
    fast_and_g32("cdecim_D2", "cdecim", 12, 9, thr(31) + pad, decim=2, phase=1, crosses=d2)
    cext("cdecim_D2_g64", "cdecim", "GENERIC64/0", 9, thr(30) + pad, x_off=1, decim=2, phase=0,
         crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "byte", 32)))
    cext("cdecim_D16_fast", "cdecim", "FAST/64", 64, thr(32) + pad, decim=16, phase=15,
         crosses=(("in", "frame", 32), ("in", "byte", 34)))
    cext("cdecim_rows_fast", "cdecim", "FAST/16", 16, W, rows=many, decim=3, phase=2, crosses=(("in", "frame", 31),))
    # rows of W + 2 frames: every other row starts 8 bytes off a 16-byte boundary, which the fast kernel does not take
    cext("cdecim_rows_generic32", "cdecim", "GENERIC32/0", 16, W + 2, rows=many, decim=3, phase=2,
         crosses=(("in", "frame", 31),))
    fast_and_g32("cinterp_U16", "cinterp", 4, 64, thr(27) + pad, up=16,
                 crosses=(("out", "frame", 31), ("out", "elem", 32), ("out", "byte", 34)))
    cext("cinterp_U2_fast", "cinterp", "FAST/6", 9, thr(30) + pad, up=2,
         crosses=(("in", "elem", 31), ("in", "byte", 32), ("out", "frame", 31)))
    cext("cinterp_rows_fast", "cinterp", "FAST/4", 16, W, rows=thr(17) + 3, up=4, crosses=(("out", "frame", 31),))
    fast_and_g32("cresample_3_2", "cresample", 24, 72, up_to(2 * thr(31), 3) + pad, up=3, decim=2, phase=1,
                 crosses=(("out", "frame", 31), ("out", "byte", 34), ("in", "byte", 32)))
    fast_and_g32("cresample_2_3", "cresample", 6, 9, thr(31) + pad, up=2, decim=3, phase=2,
                 crosses=(("in", "frame", 31), ("stuffed", "frame", 32), ("out", "elem", 31)))
    cext("cresample_rows_fast", "cresample", "FAST/8", 16, W, rows=many, up=2, decim=3, phase=1,
         crosses=(("in", "frame", 31),))
    fast_and_g32("cstream_D2", "cstream", 48, 33, thr(31) + pad, decim=2, phase=1, crosses=d2)
    cext("cstream_rows_fast", "cstream", "FAST/64", 64, W, rows=many, decim=3, phase=2,
         crosses=(("in", "frame", 31), ("hist", "frame", 24)))

    out = []
    for c in big:
        out.append(c)
        small = dict(rows=2 * Q) if c.rows > 1 else dict(width=2 * P + (pad8 - pad if c.width % 8 == 0 else 0))
        out.append(replace(c, name="twin_" + c.name, kernel=None, crosses=(), **small))
    return out


# ---- dispatch, restated ------------------------------------------------------------------------------
def rate_args(c: Case) -> tuple:
    """The rate arguments of a complex-rate family's entry, route query and predicted_route, in their order."""
    return {"cdecim": (c.decim, c.phase), "cinterp": (c.up,), "cresample": (c.up, c.decim, c.phase),
            "cstream": (c.decim, c.phase)}[c.family]


def route_name(family: str, route) -> str:
    """A library's (route, bucket) in the form of Case.kernel, e.g. "cdecim:FAST/12"."""
    return f"{family}:{ROUTES[route[0]]}/{route[1]}"


def cext_addrs(c: Case, x_ptr: int, y_ptr: int, hist_in_ptr: int = 0, hist_out_ptr: int = 0) -> tuple:
    """The address arguments of the family's route query: x and y, a stream's two histories between them."""
    return (x_ptr, hist_in_ptr, y_ptr, hist_out_ptr) if c.family == "cstream" else (x_ptr, y_ptr)


def dispatch_kernel(c: Case, x_ptr: int, y_ptr: int, hist_in_ptr: int = 4096, hist_out_ptr: int = 8192) -> str:
    """The kernel csrc launches for the case with x and y at these addresses.  The full-rate
    (``fixed``, ``bank``) and ``ideal`` branches are tests/fullrate_property_cases.py's restatement
    (rows_kernel, bank_fused, ideal_kernel), stated once there; a complex-rate family's is its
    helper's predicted_route (a stream's histories at the two further addresses)."""
    if c.family in CEXT:
        pred = CEXT[c.family][1].predicted_route(*cext_addrs(c, x_ptr, y_ptr, hist_in_ptr, hist_out_ptr), c.rows, c.width,
                                                 taps_of(c), *rate_args(c), FRAC, ACC, c.stage)
        return route_name(c.family, pred)
    u8 = c.dtype == "u8"
    rows, ch, L = c.rows, c.ch, c.taps
    h = np.asarray(taps_of(c) if c.family != "ideal" else [0], dtype=np.int64).reshape(-1)
    taps16 = bool(h.min() >= -32768 and h.max() <= 32767)
    xa = x_ptr % (8 if u8 else 16) == 0      # the alignment the LDS kernels ask of x
    if c.family == "ideal":                   # launch_fir1d_ideal
        return ideal_kernel(rows, c.width, L, x_ptr, y_ptr)
    real_ch = ch == 1 or (ch == 2 and not u8)
    if c.family == "bank":                    # launch_fir1d_rows_multi: fused u8 banks only, here
        bank = FullRateCase("bank", "fused", c.dtype, ch, c.stage, tuple(tuple(int(v) for v in r) for r in taps_of(c)), FRAC,
                            ACC, rows, c.width)
        assert bank_fused(bank, x_ptr, y_ptr)
        return "fir1d_reg_kernel"
    if c.family == "fixed":                   # launch_fir1d_rows
        return rows_kernel(u8, c.stage, ch, rows, c.width, [int(v) for v in h], x_ptr, y_ptr, FRAC, ACC)
    if c.family == "cplx":                    # launch_fir1d_cplx (no case here has every hi == 0)
        assert np.any(h.reshape(-1, 2)[:, 1] != 0)
        dot2 = bool(h.min() >= -32767 and h.max() <= 32767)
        if (L <= 64 and c.stage == I32 and dot2 and x_ptr % 16 == 0 and y_ptr % 16 == 0
                and (rows == 1 or c.width % 4 == 0) and rows * c.width < 1 << 40):
            return "fir1d_cplx_kernel"
        return "fir1d_cplx_generic32_kernel" if x_ptr % 4 == 0 and dot2 else "fir1d_cplx_generic_kernel"
    shape_ok = real_ch and taps16 and xa and (rows == 1 or (c.width * ch) % 8 == 0) and c.width < 1 << 40
    if c.family == "decim":                   # decim_path_ok
        tiles = -(-c.out_width // 512)
        fast = 2 <= c.decim <= 16 and L <= 128 and shape_ok and tiles < 1 << 31 and rows < (1 << 31) // tiles
        return "fir1d_decim_kernel" if fast else "fir1d_decim_generic_kernel"
    if c.family == "interp":                  # interp_path_ok: a workgroup owns kIntInBytes / in_size input frames
        groups = -(-c.width // (4096 // c.in_itemsize))
        fast = 2 <= c.up <= 16 and L <= 128 and shape_ok and groups < 1 << 31 and rows < (1 << 31) // groups
        return "fir1d_interp_kernel" if fast else "fir1d_interp_generic_kernel"
    assert c.family == "resample" and c.up > 1 and c.decim > 1  # U = 1 or D = 1 would be forwarded
    periods = 256                             # res_periods: kResMinT doubled up to kResInBytes of input
    while periods * c.decim * c.in_itemsize < 4096:
        periods *= 2
    groups = -(-c.out_width // (periods * c.up))
    fast = (2 <= c.up <= 16 and 2 <= c.decim <= 16 and -(-L // c.up) <= 64 and shape_ok and groups < 1 << 31
            and rows < (1 << 31) // groups)
    return "fir1d_resample_kernel" if fast else "fir1d_resample_generic_kernel"


# ---- the input ---------------------------------------------------------------------------------------
def base_of(c: Case) -> np.ndarray:
    """The samples everything is tiled from: (1, P * ch), or (Q, width * ch) for a many-rows case."""
    rng = np.random.default_rng(c.seed + 1)
    lo, hi = (0, 256) if c.dtype == "u8" else (-32768, 32768)
    shape = (c.Q, c.width * c.ch) if c.rows > 1 else (1, c.P * c.ch)
    return rng.integers(lo, hi, shape, dtype=c.np_in)


def make_x(c: Case, device) -> torch.Tensor:
    """x on ``device``: a row of width * ch samples (1-D) or (rows, width * ch), filled from a tiled
    block of whole periods, x_off elements past a 16-byte boundary."""
    base = torch.from_numpy(base_of(c)).to(device)
    n = c.in_elems
    buf = torch.empty(n + 16, dtype=c.torch_in, device=device)
    lead = (-buf.data_ptr() % 16) // c.in_itemsize + c.x_off
    flat = buf[lead:lead + n]
    assert flat.data_ptr() % 16 == c.x_off * c.in_itemsize
    unit = base.numel()                                   # one period: P * ch samples, or Q rows
    block = base.reshape(-1).repeat(max(1, FILL // unit))
    for i in range(0, n, block.numel()):
        m = min(block.numel(), n - i)
        flat[i:i + m] = block[:m]
    return flat if c.rows == 1 else flat.view(c.rows, c.width * c.ch)


def make_y(c: Case, device) -> torch.Tensor:
    """The output tensor of the entry's shape, every byte the sentinel."""
    y = torch.empty(c.out_elems, dtype=c.torch_out, device=device)
    b = y.view(torch.uint8)
    for i in range(0, b.numel(), GIB):
        b[i:i + GIB].fill_(SENTINEL)
    row = (c.rows, c.out_width * c.ch) if c.rows > 1 else (c.out_width * c.ch,)
    return y.view(((c.filters,) if c.family == "bank" else ()) + row)


def hist_base(c: Case) -> np.ndarray:
    """The histories a stream's hist_in is tiled from: (1, 2 H), or (Q, 2 H) for a many-rows case."""
    return cstream_cases.hostile_history(np.random.default_rng(c.seed + 2), c.Q if c.rows > 1 else 1, c.hist_frames)


def hist_rows(c: Case, r0: int = 0, r1: int = 1):
    """hist_in of rows r0 .. r1 - 1 as a (r1 - r0, 2 H) array (row r has history r % Q); None for
    a family without one."""
    if not c.hist_frames:
        return None
    base = hist_base(c)
    return base[np.arange(r0, r1) % base.shape[0]]


def make_hist(c: Case, device) -> torch.Tensor:
    """A stream's hist_in on ``device``: (2 H,) for one row, else (rows, 2 H)."""
    base = torch.from_numpy(hist_base(c)).to(device)
    if c.rows == 1:
        return base.reshape(-1).clone()
    return base.repeat(-(-c.rows // c.Q), 1)[:c.rows].contiguous()


# ---- the references ------------------------------------------------------------------------------------
def reference(c: Case, x: np.ndarray, hist: np.ndarray | None = None) -> np.ndarray:
    """What the family's entry must give for the (rows, width' * ch) array x: (rows, out_width' * ch),
    a bank (filters, rows, ...); the references of the families' own GPU tests.  hist: a stream's
    (rows, 2 H) history before x (None: zeros)."""
    h = taps_of(c)
    if c.family == "cdecim":
        return cdecim_cases.want(x, h, c.decim, c.phase, FRAC, ACC, c.stage)
    if c.family == "cinterp":
        return cinterp_cases.want(x, h, c.up, FRAC, ACC, c.stage)
    if c.family == "cresample":
        return cresample_cases.want(x, h, c.up, c.decim, c.phase, FRAC, ACC, c.stage)
    if c.family == "cstream":
        return cstream_cases.want_block(x, hist, h, c.decim, c.phase, FRAC, ACC, c.stage)[0]
    o = c_oracle()
    if c.family == "fixed":
        return o.fir1d_rows(x, h, FRAC, ACC, c.stage, channels=c.ch)
    if c.family == "bank":
        return np.stack([o.fir1d_rows(x, hf, FRAC, ACC, c.stage, channels=c.ch) for hf in h])
    if c.family == "ideal":
        return o.fir1d_ideal_rows(x, h)
    if c.family == "decim":
        return decim_want(x, h, c.decim, c.phase, FRAC, ACC, c.stage, c.ch).reshape(x.shape[0], -1)
    if c.family == "interp":
        return interp_want(x, h, c.up, FRAC, ACC, c.stage, c.ch)
    if c.family == "resample":
        return resample_want(x, h, c.up, c.decim, c.phase, FRAC, ACC, c.stage, c.ch)
    return cplx_ref.want(x, h, FRAC, ACC, c.stage)


def input_span(c: Case, out_lo: int, out_hi: int) -> tuple[int, int, int]:
    """(lo, hi, q): the input frames [lo, hi) of a single row whose reference holds output frames
    [out_lo, out_hi) exactly, local output m' being global output q + m'.  Output m reads the
    stuffed signal around index m * D + phase, i.e. input frames within taps / U of it: a lead-in
    and a lead-out of taps + D + 8 input frames cover that (or the slice ends at the row's own end,
    where the zero padding is the true one).  lo is a multiple of D, so lo * U is one and
    [phase::D] of the slice lines up with that of the row."""
    U, D = c.up, c.decim
    lead = c.taps + D + 8
    lo = max(0, out_lo * D // U - lead)
    lo -= lo % D
    hi = min(c.width, -(-(out_hi * D + c.phase) // U) + lead)
    return lo, hi, lo * U // D


# ---- the comparisons -------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    """verify's finding: .step ("periods" | "rows" | "band" | "hist"), .index (the first differing
    output element; of hist_out for "hist"), .frame (its frame, counted from the tensor's start) and
    .count."""

    def __init__(self, c: Case, step: str, index: int, count: int, of: int, detail: str = ""):
        self.step, self.index, self.count = step, index, count
        self.frame = index // c.ch
        what, itemsize = ("hist_out", c.in_itemsize) if step == "hist" else ("output", c.out_itemsize)
        super().__init__(f"{c.name} [{step}]: {count} of {of} compared {what} values differ{detail}; the first is {what} "
                         f"frame {self.frame} (element {index}, byte offset {index * itemsize:#x})")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64) if t.dtype == torch.float64 else t  # float64 is compared bit for bit


def _diff(a: torch.Tensor, b: torch.Tensor) -> tuple[int, int]:
    """(differing elements, flat index of the first in a) of a against b (broadcast); at most CHUNK
    elements, so the temporaries are a bool and a uint8 of that many."""
    ne = torch.ne(a, b)
    count = int(ne.count_nonzero())
    return (count, int(torch.argmax(ne.reshape(-1).to(torch.uint8)))) if count else (0, -1)


def compare_periods(c: Case, y: torch.Tensor, chunk: int = CHUNK) -> None:
    """Step 3, one row: every output frame from period 2 on, up to the row end's own edge, against
    period 1."""
    yb = _bits(y.reshape(-1))
    Te = c.period * c.ch
    edge = ((c.taps // 2 + 1) * c.up // c.decim + 2) * c.ch  # outputs that see the zero padding past the row's end
    hi = yb.numel() - edge
    ref = yb[Te:2 * Te]
    count, first, m = 0, -1, max(1, chunk // Te)
    s = 2 * Te
    while s < hi:
        k = min(m, (hi - s) // Te)
        if k:
            n, i = _diff(yb[s:s + k * Te].view(k, Te), ref)
        else:  # the ragged last period
            n, i = _diff(yb[s:hi], ref[:hi - s])
        if n and first < 0:
            first = s + i
        count += n
        s = s + k * Te if k else hi
    if count:
        raise Mismatch(c, "periods", first, count, hi - 2 * Te, f" from output frame {first // c.ch % c.period} of period 1")


def compare_rows(c: Case, y: torch.Tensor, chunk: int = CHUNK) -> None:
    """Step 3, many rows: every output row r >= Q against row r % Q, each plane of a bank."""
    We = c.out_width * c.ch
    planes = _bits(y).reshape(c.filters, c.rows, We)
    count, first, m = 0, -1, max(1, chunk // (c.Q * We))
    for f in range(c.filters):
        yb = planes[f]
        ref = yb[:c.Q]
        r0 = c.Q
        while r0 < c.rows:
            k = min(m, (c.rows - r0) // c.Q)
            if k:
                n, i = _diff(yb[r0:r0 + k * c.Q].view(k, c.Q, We), ref)
            else:  # the last, partial run of rows
                n, i = _diff(yb[r0:], ref[:c.rows - r0])
            if n and first < 0:
                first = (f * c.rows + r0) * We + i
            count += n
            r0 = r0 + k * c.Q if k else c.rows
    if count:
        raise Mismatch(c, "rows", first, count, c.filters * max(0, c.rows - c.Q) * We,
                       f" from row {first // We % c.rows % c.Q} of the first {c.Q}")


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def _band_diff(c: Case, got: np.ndarray, want: np.ndarray, base: int, what: str) -> None:
    """got / want: equal-shaped arrays whose flat element i is output element base + i."""
    if got.dtype == np.float64:
        got, want = got.view(np.int64), want.view(np.int64)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if bad.size:
        raise Mismatch(c, "band", base + int(bad[0]), int(bad.size), got.size, f" from the reference ({what})")


def compare_bands(c: Case, x: torch.Tensor, y: torch.Tensor) -> None:
    """Step 4: periods 0-1 and the last two periods with the ragged tail (rows 0 .. Q-1 and the last Q
    rows) against the reference of the matching slice of x."""
    if c.rows > 1:
        We = c.out_width * c.ch
        spans = [(0, c.rows)] if c.rows <= 2 * c.Q else [(0, c.Q), (c.rows - c.Q, c.rows)]
        y3 = y.reshape(c.filters, c.rows, We)
        for r0, r1 in spans:
            want = reference(c, _host(x[r0:r1]), hist_rows(c, r0, r1)).reshape(c.filters, r1 - r0, We)
            for f in range(c.filters):
                _band_diff(c, _host(y3[f, r0:r1]), want[f], (f * c.rows + r0) * We, f"rows {r0} .. {r1 - 1}")
        return
    T, n_out = c.period, c.out_width
    full = n_out // T
    spans = [(0, n_out)] if full < 5 else [(0, 2 * T), ((full - 2) * T, n_out)]
    xf, yf = x.reshape(-1), y.reshape(-1)
    for out_lo, out_hi in spans:
        lo, hi, q = input_span(c, out_lo, out_hi)
        # a stream's slice from frame 0 has the row's history before it; a later one a lead-in that is thrown away
        want = reference(c, _host(xf[lo * c.ch:hi * c.ch]).reshape(1, -1), hist_rows(c) if lo == 0 else None).reshape(-1)
        _band_diff(c, _host(yf[out_lo * c.ch:out_hi * c.ch]), want[(out_lo - q) * c.ch:(out_hi - q) * c.ch],
                   out_lo * c.ch, f"output frames {out_lo} .. {out_hi - 1} from input frames {lo} .. {hi - 1}")


def compare_hist(c: Case, x: torch.Tensor, hist_out: torch.Tensor) -> None:
    """A stream's hist_out against the last H frames of every row of x, bit for bit, on the device
    (every case here has rows of H frames and more, so none of hist_in remains in it)."""
    He = c.hist_frames * c.ch
    assert c.width >= c.hist_frames and hist_out.numel() == c.rows * He <= CHUNK
    n, i = _diff(hist_out.reshape(c.rows, He), x.reshape(c.rows, -1)[:, c.width * c.ch - He:])
    if n:
        raise Mismatch(c, "hist", i, n, c.rows * He, f" from the last {c.hist_frames} frames of x (row {i // He})")


def verify(c: Case, x: torch.Tensor, y: torch.Tensor, chunk: int = CHUNK, hist_out: torch.Tensor | None = None) -> None:
    """Steps 3 and 4 on the entry's output y for the input x; raises Mismatch.  The bands go first:
    period 1 and rows 0 .. Q-1 are what step 3 compares everything else with, so an error there is
    named where it is and not where its first copy was expected.  A stream's hist_out is held
    against x between the two."""
    compare_bands(c, x, y)
    if c.hist_frames:
        compare_hist(c, x, hist_out)
    if c.rows > 1:
        compare_rows(c, y, chunk)
    else:
        compare_periods(c, y, chunk)
