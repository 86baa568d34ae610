"""Hypothesis strategies, dispatch restatements and references for the full-rate and 2-D FIR
families -- a test helper, not a test module.

tests/test_gpu_property_fullrate.py runs the strategies on the GPU through the DEVICE entries;
tests/test_fullrate_property_cases.py keeps this module honest without one.  The families and
their entries (all in fir_hip.torch_ops):

    rows     fir1d_fixed_rows_dev                                       csrc/fir1d.hip (launch_fir1d_rows)
    bank     fir1d_fixed_rows_multi_dev                                 csrc/fir1d.hip (launch_fir1d_rows_multi)
    images   fir1d_fixed_images_multi_dev, ImagesMultiPlan.launch       csrc/fir1d.hip (launch_fir1d_images_multi)
    segment  fir1d_fixed_segment_dev; fir1d_fixed_rows_dev + _edges_dev csrc/fir1d.hip (launch_fir1d_segment / _edges)
    fir2d    fir2d_fixed_dev (FIR2D_PATH unset / reg / mfma)            csrc/fir2d.hip, fir2d_mfma.hip
    ideal    fir1d_ideal_rows_dev, fir2d_ideal_dev                      csrc/ideal.hip, ideal2d.hip

References: the committed C oracle (fir1d_rows with channels and halos, fir2d, fir1d_ideal_rows)
and tests/ideal2d_ref.ideal2d; every comparison is bit for bit.

Routes, by construction.  A strategy first draws the route it intends and then builds a call that
takes it: no assume(), no .filter().  ``route_of`` restates the dispatchers on real addresses and
``launches_of`` gives the kernels the call must log, in order.  Where a call leaves every fast
kernel for ``fir1d_generic_kernel`` the route names the first reason, in one fixed order (taps,
bits, channels, shape, align), that no kernel of the call's tap count accepts; a strategy that
intends ``generic:X`` switches X on, every reason before X off and each reason after X on in
about one draw of four.

    rows     reg | mfma_step | mfma_run (u8) | mfma_long (int16) | lds |
             generic:taps      a tap outside the range its length's kernel takes (1-9 taps: 24 bits;
                               10-64: int16; 65 and up: [-32768, 32639], the matrix-core split)
             generic:bits      acc_bits > 32 or frac_bits > 31
             generic:channels  3 channels, 2 channels of u8; 2 channels past 9 taps
             generic:shape     several rows shorter than a vector plus the halo (1-9 taps) or of no
                               multiple of 8 samples (10 and up); past 64 taps also one such row
             generic:align     x off 16 bytes (past 9 taps: u8 off 8), y off 16 bytes
             (``lds`` also holds the calls of 2-9 taps that miss the register kernel by shape or by
             a u8 x at 8 mod 16 and still suit the LDS kernel.)
    bank     fused (ceil(F / 4) launches of fir1d_reg_kernel) | each (F calls of the rows dispatcher,
             plane f at its own address)
    images   batch | single | mixed: what the call's non-empty images take (a call without one is
             named by what its filters and types alone allow).  The log holds each single image's F
             rows launches in image order, then ceil(B / 8) ceil(F / 4) fir1d_reg_batch_kernel
             launches for the B batch images.
    segment  one (register kernel with halos) | rows+edges (any rows kernel, then fir1d_edges_kernel;
             a 1-tap filter has no edge and no second launch) | all_edge (a segment no longer than
             its halos: the rows kernel of the bare segment, then fir1d_generic_kernel with halos)
    fir2d    mfma | pk16_strip | reg | generic
    ideal    1d:reg | 1d:generic | 2d:reg | 2d:generic

Sizes.  A reference costs rows * width * channels * taps multiply-adds on the host, so a drawn
width is capped at rate_property_cases.WORK of them (by min(), not by rejection): the 2100-tap
filters meet rows of a few matrix-core tiles, every filter up to a few hundred taps meets rows
past two workgroups.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np
from hypothesis import strategies as st

import fir_hip
import range_cases as rg
from ideal2d_ref import ideal2d
from oracle import c_oracle
from rate_property_cases import _POKE_REAL, _SEED, WORK, _bits, _tap_values

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
FAMILIES = ("rows", "bank", "images", "segment", "fir2d", "ideal")

# The constants of csrc restated here, with the file each lives in
# (tests/test_fullrate_property_cases.py reads them back).
LIMITS = {
    "kMfmaMinTaps": ("fir1d.hip", 10), "kMfmaMinTapsI32": ("fir1d.hip", 40), "kGenTile": ("fir1d.hip", 1024),
    "kLdsMaxTaps": ("fir1d_lds.hip", 64), "kLdsVec": ("fir1d_lds.hip", 8),
    "kMfTile": ("fir1d_mfma.hip", 1024), "kMfMaxTaps": ("fir1d_mfma.hip", 65536), "kMf2Blocks": ("fir1d_mfma.hip", 2048),
    "kMrC": ("fir1d_mfma.hip", 16), "kMrU8One": ("fir1d_mfma.hip", 32), "kMlChunk": ("fir1d_mfma.hip", 16),
    "kRegBatch": ("fir1d_reg_launch.h", 8), "kBlock": ("fir_common.h", 256), "kWave": ("fir_common.h", 64),
    "kVec2d": ("fir2d.hip", 16), "kStrip2dSep": ("fir2d.hip", 16),
    "kM2MaxR": ("fir2d_mfma.hip", 7), "kM2MaxC": ("fir2d_mfma.hip", 5),
    "kIdealNV": ("ideal.hip", 1), "kIdeal2dMaxRC": ("ideal2d.hip", 5),
}
REG_MAX_TAPS = 9                      # "L <= 9" of reg_path_ok and launch_fir1d_ideal
MFMA_MIN, MFMA_MIN_I32 = 10, 40       # kMfmaMinTaps, kMfmaMinTapsI32
LDS_MAX_TAPS, LDS_VEC = 64, 8         # kLdsMaxTaps, kLdsVec
MF_TILE, MF_MAX_TAPS = 1024, 65536    # kMfTile, kMfMaxTaps
REG_BATCH = 8                         # kRegBatch
VEC2D, STRIP2D = 16, 16               # kVec2d, kStrip2dSep
IDEAL2D_MAX = 5                       # kIdeal2dMaxRC
MAX_LEN = 2100                        # the longest drawn filter
TALL_H = 65535 * STRIP2D              # the tallest frame of the 2-D register kernels: gridDim.y = 65535

REG, STEP, RUN, LONG = "fir1d_reg_kernel", "fir1d_mfma_step_kernel", "fir1d_mfma_run_kernel", "fir1d_mfma_long_kernel"
LDS, GENERIC, EDGES, BATCH = "fir1d_lds_kernel", "fir1d_generic_kernel", "fir1d_edges_kernel", "fir1d_reg_batch_kernel"
ROWS_ROUTE = {REG: "reg", STEP: "mfma_step", RUN: "mfma_run", LONG: "mfma_long", LDS: "lds"}
KERNEL_2D = {"mfma": "fir2d_mfma_kernel", "pk16_strip": "fir2d_pk16_strip_kernel", "reg": "fir2d_reg_kernel",
             "generic": "fir2d_generic_kernel"}
KERNEL_IDEAL = {"1d:reg": "fir1d_ideal_reg_kernel", "1d:generic": "fir1d_ideal_kernel",
                "2d:reg": "fir2d_ideal_reg_kernel", "2d:generic": "fir2d_ideal_generic_kernel"}

ROUTES = {
    "rows": ("reg", "mfma_step", "mfma_run", "mfma_long", "lds", "generic:taps", "generic:bits", "generic:channels",
             "generic:shape", "generic:align"),
    "bank": ("fused", "each"),
    "images": ("batch", "single", "mixed"),
    "segment": ("one", "rows+edges", "all_edge"),
    "fir2d": ("mfma", "pk16_strip", "reg", "generic"),
    "ideal": ("1d:reg", "1d:generic", "2d:reg", "2d:generic"),
}


@dataclass(frozen=True)
class Image:
    """One image of an ``images`` call; y_leads: the byte lead of each of its F output planes."""
    rows: int
    width: int
    x_lead: int = 0
    y_leads: tuple = (0,)


@dataclass(frozen=True)
class Case:
    """One call.  hq: the taps -- rows / segment: ints; bank / images: F tuples of ints; fir2d: R
    tuples of C ints; ideal: floats (1d:*) or R tuples of C floats (2d:*).  rows, width: the rows and
    frames per row of x (segment: one row of ``width`` frames; 2-D: H, W).  frames: 0 for one 2-D
    frame, else the batch's frames.  x_lead / y_lead (halos: hl_lead / hr_lead): bytes past a
    512-byte boundary at which guarded_input / guarded_output place the tensors.  halos: which of
    the segment's two halos is a tensor (the other is None: zeros).  path: FIR2D_PATH."""
    family: str
    route: str
    dtype: str = "u8"  # "u8" | "i16"
    ch: int = 1
    stage: int = U8
    hq: tuple = (4096,)
    frac: int = 12
    acc: int = 32
    rows: int = 1
    width: int = 64
    frames: int = 0
    seed: int = 0
    fill: str = "uniform"  # "uniform" | "ends" | "min" | "max"
    x_lead: int = 0
    y_lead: int = 0
    halos: tuple = (True, True)
    hl_lead: int = 0
    hr_lead: int = 0
    path: str | None = None
    images: tuple = ()

    @property
    def np_dtype(self):
        return np.uint8 if self.dtype == "u8" else np.int16

    @property
    def u8(self) -> bool:
        return self.dtype == "u8"

    @property
    def in_itemsize(self) -> int:
        return 1 if self.u8 else 2

    @property
    def out_itemsize(self) -> int:
        return 8 if self.family == "ideal" else (4 if self.stage == I32 else 1)

    @property
    def filters(self) -> int:
        return len(self.hq) if self.family in ("bank", "images") else 1

    @property
    def taps(self) -> int:
        """Taps per filter (2-D: R * C)."""
        if self.family in ("bank", "images"):
            return len(self.hq[0])
        if self.family == "fir2d" or self.route.startswith("2d"):
            return len(self.hq) * len(self.hq[0])
        return len(self.hq)

    @property
    def halo_sizes(self) -> tuple:
        """Samples of the segment's left and right halo: (L - 1 - L // 2) * ch, (L // 2) * ch."""
        L = len(self.hq)
        return (L - 1 - L // 2) * self.ch, (L // 2) * self.ch

    @property
    def work(self) -> int:
        """Multiply-adds of the case's reference."""
        if self.family == "images":
            return sum(i.rows * i.width for i in self.images) * self.ch * self.taps * self.filters
        return max(self.frames, 1) * self.rows * self.width * self.ch * self.taps * self.filters


# ---- samples -------------------------------------------------------------------------------------
def _fill(rng, shape, dtype, fill):
    lo, hi = (0, 255) if dtype == np.uint8 else (-32768, 32767)
    if fill == "uniform":
        return rng.integers(lo, hi + 1, shape, dtype=dtype)
    if fill == "ends":
        return np.where(rng.integers(0, 2, shape) == 0, lo, hi).astype(dtype)
    return np.full(shape, lo if fill == "min" else hi, dtype)


def samples(c: Case, again: int = 0):
    """The input of a case from its seed: rows / bank / ideal 1-D: (rows, width * ch); segment: (x,
    halo_left, halo_right), an absent or empty halo None; images: a list of (rows_i, width_i * ch);
    2-D: (H, W) or (frames, H, W).  ``again``: another draw of the same shapes (the second launch
    of an ImagesMultiPlan)."""
    rng = np.random.default_rng([c.seed, again])
    if c.family == "images":
        return [_fill(rng, (i.rows, i.width * c.ch), c.np_dtype, c.fill) for i in c.images]
    if c.family == "fir2d" or c.route.startswith("2d"):
        return _fill(rng, ((c.frames,) if c.frames else ()) + (c.rows, c.width), np.uint8, c.fill)
    if c.family == "segment":
        x = _fill(rng, (c.width * c.ch,), c.np_dtype, c.fill)
        hl, hr = (_fill(rng, (n,), c.np_dtype, c.fill) if on and n else None for on, n in zip(c.halos, c.halo_sizes))
        return x, hl, hr
    return _fill(rng, (c.rows, c.width * c.ch), np.uint8 if c.family == "ideal" else c.np_dtype, c.fill)


# ---- references ----------------------------------------------------------------------------------
def _rows_ref(x, h, c: Case, **halos):
    if x.size == 0:  # the oracle takes no empty array
        return np.zeros(x.shape, np.uint8 if c.stage == U8 else np.int32)
    return c_oracle().fir1d_rows(x, h, c.frac, c.acc, c.stage, channels=c.ch, **halos)


def want(c: Case, x):
    """What the family's entry must give for ``samples(c)``: an array of the output's shape (bank:
    (F, rows, width * ch); images: a list of (F, rows_i, width_i * ch))."""
    if c.family == "rows":
        return _rows_ref(x, c.hq, c)
    if c.family == "bank":
        return np.stack([_rows_ref(x, h, c) for h in c.hq])
    if c.family == "images":
        return [np.stack([_rows_ref(xi, h, c) for h in c.hq]) for xi in x]
    if c.family == "segment":
        xs, hl, hr = x
        return _rows_ref(xs, c.hq, c, halo_left=hl, halo_right=hr)
    if c.family == "fir2d":
        h2 = np.asarray(c.hq, dtype=np.int64)
        one = lambda f: c_oracle().fir2d(f, h2, c.frac, c.acc, c.stage)  # noqa: E731
    elif c.route.startswith("2d"):
        one = lambda f: ideal2d(f, np.asarray(c.hq, dtype=np.float64))  # noqa: E731
    else:
        return c_oracle().fir1d_ideal_rows(x, np.asarray(c.hq, dtype=np.float64))
    return np.stack([one(f) for f in x]) if c.frames else one(x)


def describe_mismatch(c: Case, got: np.ndarray, ref: np.ndarray, what: str = "") -> str | None:
    """None when got equals ref bit for bit (float64 as uint64 views); else where the first
    difference is, in the output's own coordinates, with the drawn route."""
    head = f"{c.family} [{c.route}]{what}: "
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"{head}got {got.shape} {got.dtype}, want {ref.shape} {ref.dtype}; {c}"
    a, b = (got.view(np.uint64), ref.view(np.uint64)) if ref.dtype == np.float64 else (got, ref)
    if np.array_equal(a, b):
        return None
    bad = np.argwhere(a != b)
    at = tuple(int(v) for v in bad[0])
    names = {"rows": ("row", "sample"), "segment": ("sample",), "bank": ("filter", "row", "sample"),
             "images": ("filter", "row", "sample")}.get(c.family, ("frame", "row", "column")[-len(at):])
    where = ", ".join(f"{n} {v}" for n, v in zip(names, at))
    if c.family in ("rows", "segment", "bank", "images") and c.ch > 1:
        where += f" (frame {at[-1] // c.ch}, channel {at[-1] % c.ch})"
    return f"{head}{len(bad)} of {ref.size} values differ; the first at {where}: got {got[at]!r}, want {ref[at]!r}; {c}"


# ---- the dispatchers, restated ---------------------------------------------------------------------
def _mfma_ksteps(L: int) -> int:
    """launch_mfma_t (fir1d_mfma.hip): the 32-tap k-steps of an L-tap filter, its halo rounded to 8."""
    c = L // 2
    hl = L - 1 - c
    return (32 + c + ((hl + 7) & ~7) + 31) // 32


def _mfma_ksteps16(L: int) -> int:
    """The run kernel's own count: the halo rounded to 16 (launch_mfma_t, the u8 branch)."""
    c = L // 2
    hl = L - 1 - c
    return (32 + c + ((hl + 15) & ~15) + 31) // 32


def reg_ok(u8: bool, ch: int, rows: int, rowlen: int, taps, L: int, x_ptr: int, y_ptr: int, frac: int, acc: int) -> bool:
    """reg_path_ok (fir1d.hip); ``taps``: every tap the launch holds (a bank: F * L of them)."""
    vec = 16 if u8 else 8
    return (L <= REG_MAX_TAPS and (ch == 1 or (ch == 2 and not u8)) and acc <= 32 and frac <= 31
            and min(taps) >= -(1 << 23) and max(taps) < 1 << 23 and x_ptr % 16 == 0 and y_ptr % 16 == 0
            and (rows == 1 or (rowlen >= vec + (L - 1) * ch and rows * rowlen < 1 << 32)))


def rows_kernel(u8: bool, stage: int, ch: int, rows: int, width: int, h, x_ptr: int, y_ptr: int, frac: int = 12,
                acc: int = 32) -> str:
    """The kernel launch_fir1d_rows (fir1d.hip) launches for a non-empty call: reg_path_ok, then
    mfma_path_ok past kMfmaMinTaps / kMfmaMinTapsI32 with the k-step count of launch_mfma_t, then
    lds_path_ok, else the generic kernel."""
    L, rowlen = len(h), width * ch
    total = rows * rowlen
    lo, hi = min(h), max(h)
    if reg_ok(u8, ch, rows, rowlen, h, L, x_ptr, y_ptr, frac, acc):
        return REG
    bits = acc <= 32 and frac <= 31
    aligned = x_ptr % (8 if u8 else 16) == 0 and y_ptr % 16 == 0
    ntiles = rows * (-(-rowlen // MF_TILE)) if rows > 1 else -(-total // MF_TILE)
    mfma = (2 <= L <= MF_MAX_TAPS and ch == 1 and lo >= -32768 and hi <= 32639 and bits
            and (total if rows == 1 else rowlen) % 8 == 0 and aligned and 8 <= total < 1 << 40
            and ntiles < (1 << 32) - 2048 * 4)
    if L >= (MFMA_MIN_I32 if not u8 and stage == I32 else MFMA_MIN) and mfma:
        if _mfma_ksteps(L) <= 3:
            return STEP
        return RUN if u8 else LONG
    lds = (2 <= L <= LDS_MAX_TAPS and ch == 1 and lo >= -32768 and hi <= 32767 and bits
           and (rows == 1 or rowlen % LDS_VEC == 0) and aligned and total < 1 << 40)
    return LDS if lds else GENERIC


def generic_reasons(u8: bool, ch: int, rows: int, width: int, h, x_ptr: int, y_ptr: int, frac: int, acc: int) -> list:
    """Why no kernel of the call's tap count takes it, in this module's order."""
    L, rowlen = len(h), width * ch
    total = rows * rowlen
    lo, hi = min(h), max(h)
    why = []
    if L <= REG_MAX_TAPS:
        taps_ok = lo >= -(1 << 23) and hi < 1 << 23
        ch_ok = ch == 1 or (ch == 2 and not u8)
        shape_ok = rows == 1 or (rowlen >= (16 if u8 else 8) + (L - 1) * ch and total < 1 << 32)
        x_ok = x_ptr % 16 == 0
    else:
        taps_ok = lo >= -32768 and hi <= (32767 if L <= LDS_MAX_TAPS else 32639)
        ch_ok = ch == 1
        shape_ok = rowlen % 8 == 0 if rows > 1 else (L <= LDS_MAX_TAPS or (total % 8 == 0 and total >= 8))
        x_ok = x_ptr % (8 if u8 else 16) == 0
    for name, ok in (("taps", taps_ok), ("bits", acc <= 32 and frac <= 31), ("channels", ch_ok), ("shape", shape_ok),
                     ("align", x_ok and y_ptr % 16 == 0)):
        if not ok:
            why.append("generic:" + name)
    return why


def rows_route(c: Case, x_ptr: int, y_ptr: int) -> str:
    k = rows_kernel(c.u8, c.stage, c.ch, c.rows, c.width, c.hq, x_ptr, y_ptr, c.frac, c.acc)
    if k != GENERIC:
        return ROWS_ROUTE[k]
    why = generic_reasons(c.u8, c.ch, c.rows, c.width, c.hq, x_ptr, y_ptr, c.frac, c.acc)
    assert why, ("the generic kernel for no stated reason", c)
    return why[0]


def bank_fused(c: Case, x_ptr: int, y_ptr: int) -> bool:
    """launch_fir1d_rows_multi (fir1d.hip): u8 planes may start at any byte, int32 planes on 16."""
    total = c.rows * c.width * c.ch
    flat = [v for h in c.hq for v in h]
    return (c.u8 and c.ch == 1 and (c.stage == U8 or total * 4 % 16 == 0)
            and reg_ok(True, 1, c.rows, c.width, flat, len(c.hq[0]), x_ptr, x_ptr if c.stage == U8 else y_ptr, c.frac, c.acc))


def image_batches(c: Case, im: Image, x_ptr: int) -> bool:
    """launch_fir1d_images_multi (fir1d.hip): only the image's own alignment and shape decide."""
    flat = [v for h in c.hq for v in h]
    return (c.u8 and c.ch == 1 and c.stage == U8
            and reg_ok(True, 1, im.rows, im.width, flat, len(c.hq[0]), x_ptr, x_ptr, c.frac, c.acc))


def segment_one(c: Case, x_ptr: int, y_ptr: int) -> bool:
    """launch_fir1d_segment (fir1d.hip): one launch for whole wave tiles on the register kernel."""
    total = c.width * c.ch
    return total % (4096 if c.u8 else 512) == 0 and reg_ok(c.u8, c.ch, 1, total, c.hq, len(c.hq), x_ptr, y_ptr, c.frac, c.acc)


def sep2d_register_form(h2) -> bool:
    """fir2d.hip: a rank-1 kernel of a register shape keeps the separable register kernels."""
    R, C = len(h2), len(h2[0])
    return R in (3, 5) and C in (3, 5) and rg.rank1_factor(h2) is not None


def fir2d_route(c: Case, x_ptr: int, y_ptr: int) -> str:
    """launch_fir2d (fir2d.hip) with launch_fir2d_mfma / plan_mfma2 (fir2d_mfma.hip) and the
    packed-16 plan of launch2d_reg (tests/range_cases.py restates both plans)."""
    h2 = np.asarray(c.hq, dtype=np.int64)
    R, C = h2.shape
    H, W = c.rows, c.width
    aligned = x_ptr % 16 == 0 and y_ptr % 16 == 0
    fast = (R in (1, 3, 5) and C in (1, 3, 5) and W % VEC2D == 0 and aligned and c.acc <= 32 and c.frac <= 31
            and rg.taps16(h2) and W >= VEC2D and H <= TALL_H)
    if c.path != "reg" and (c.path == "mfma" or not sep2d_register_form(c.hq)):
        if c.stage == U8 and W % 16 == 0 and W >= 16 and aligned and rg.mfma2_plan(h2, c.frac, c.acc)["np"]:
            return "mfma"
    if not fast:
        return "generic"
    strip = (c.stage == U8 and rg.sep_form(h2, c.frac, c.acc) != "general" and rg.pk16_2d(h2, c.frac, c.acc)["mode"] != 0
             and H * W < 1 << 31)
    return "pk16_strip" if strip else "reg"


def ideal_kernel(rows: int, width: int, L: int, x_ptr: int, y_ptr: int) -> str:
    """launch_fir1d_ideal (ideal.hip)."""
    total = rows * width
    reg = (L <= REG_MAX_TAPS and x_ptr % 4 == 0 and y_ptr % 16 == 0
           and (rows == 1 or (width >= 4 + L - 1 and total < 1 << 32)) and (total + 3) // 4 // 256 < 1 << 31)
    return KERNEL_IDEAL["1d:reg" if reg else "1d:generic"]


def ideal_route(c: Case, x_ptr: int, y_ptr: int) -> str:
    if c.route.startswith("1d"):
        return "1d:reg" if ideal_kernel(c.rows, c.width, len(c.hq), x_ptr, y_ptr) == KERNEL_IDEAL["1d:reg"] else "1d:generic"
    R, C, W = len(c.hq), len(c.hq[0]), c.width  # launch_fir2d_ideal (ideal2d.hip)
    reg = R <= IDEAL2D_MAX and C <= IDEAL2D_MAX and x_ptr % 4 == 0 and y_ptr % 16 == 0 and W % 4 == 0 and W >= 4 + C - 1
    return "2d:reg" if reg else "2d:generic"


def _plane(c: Case, y_ptr: int, f: int) -> int:
    return y_ptr + f * c.rows * c.width * c.ch * c.out_itemsize


def _addrs(c: Case, x_addr, y_addr):
    """The drawn leads stand for the addresses that are not given (every test of the dispatchers
    is modulo 16 or less, and a lead is the address modulo 512)."""
    if c.family == "images":
        return ([i.x_lead for i in c.images] if x_addr is None else x_addr,
                [list(i.y_leads) for i in c.images] if y_addr is None else y_addr)
    return c.x_lead if x_addr is None else x_addr, c.y_lead if y_addr is None else y_addr


def route_of(c: Case, x_addr=None, y_addr=None) -> str:
    """The route the family's dispatcher takes with x and y at these addresses (images: a list of
    image addresses and a list of each image's F plane addresses)."""
    x, y = _addrs(c, x_addr, y_addr)
    if c.family == "rows":
        return rows_route(c, x, y)
    if c.family == "bank":
        return "fused" if bank_fused(c, x, y) else "each"
    if c.family == "segment":
        if segment_one(c, x, y):
            return "one"
        return "all_edge" if c.width * c.ch <= sum(c.halo_sizes) else "rows+edges"
    if c.family == "fir2d":
        return fir2d_route(c, x, y)
    if c.family == "ideal":
        return ideal_route(c, x, y)
    kinds = {image_batches(c, im, xa) for im, xa in zip(c.images, x) if im.rows * im.width}
    if not kinds:  # nothing to run: what the call's filters and types alone allow
        kinds = {image_batches(c, Image(1, 64), 0)}
    return "mixed" if len(kinds) == 2 else ("batch" if True in kinds else "single")


def launches_of(c: Case, x_addr=None, y_addr=None) -> list:
    """The kernels the call must log, in order; an empty output launches nothing."""
    x, y = _addrs(c, x_addr, y_addr)
    if c.family == "images":
        out, batch = [], 0
        for im, xa, ya in zip(c.images, x, y):
            if not im.rows * im.width:
                continue
            if image_batches(c, im, xa):
                batch += 1
                continue
            out += [rows_kernel(c.u8, c.stage, c.ch, im.rows, im.width, h, xa, yf, c.frac, c.acc) for h, yf in zip(c.hq, ya)]
        return out + [BATCH] * (-(-batch // REG_BATCH) * -(-c.filters // 4))
    if not max(c.frames, 1) * c.rows * c.width:
        return []
    if c.family == "rows":
        return [rows_kernel(c.u8, c.stage, c.ch, c.rows, c.width, c.hq, x, y, c.frac, c.acc)]
    if c.family == "bank":
        if bank_fused(c, x, y):
            return [REG] * -(-c.filters // 4)
        return [rows_kernel(c.u8, c.stage, c.ch, c.rows, c.width, h, x, _plane(c, y, f), c.frac, c.acc)
                for f, h in enumerate(c.hq)]
    if c.family == "segment":
        if segment_one(c, x, y):
            return [REG]
        first = [rows_kernel(c.u8, c.stage, c.ch, 1, c.width, c.hq, x, y, c.frac, c.acc)]
        if c.width * c.ch <= sum(c.halo_sizes):
            return first + [GENERIC]
        return first + ([EDGES] if len(c.hq) > 1 else [])
    if c.family == "fir2d":
        return [KERNEL_2D[fir2d_route(c, x, y)]]
    return [KERNEL_IDEAL[ideal_route(c, x, y)]]


def check_sizes(c: Case) -> str | None:
    """check_fir1d (fir1d.hip), check_fir1d_ideal (ideal.hip), check_fir2d (fir2d.hip) and
    check_fir2d_ideal (ideal2d.hip): the refusal's text, None for a legal call."""
    if c.family == "ideal" and c.route.startswith("1d"):
        if c.rows < 0 or c.width < 0:
            return "rows and width must be >= 0"
        return None if 1 <= len(c.hq) <= fir_hip.MAX_TAPS else "taps"
    if c.family == "fir2d" or c.family == "ideal":
        if c.family == "fir2d" and c.stage not in (U8, I32):
            return "out_stage"
        if c.rows < 0 or c.width < 0 or c.frames < 0:
            return "frames, height and width must be >= 0"
        if c.frames > 65535:
            return "frames must be <= 65535 per call"
        R, C = len(c.hq), len(c.hq[0])
        if R < 1 or C < 1 or R * C > fir_hip.MAX_TAPS:
            return "tap_rows*tap_cols"
        if c.family == "fir2d":
            flat = [v for r in c.hq for v in r]
            if min(flat) < -(1 << 31) or max(flat) >= 1 << 31:
                return "taps"
            if c.frac < 1 or c.acc < 1:
                return "frac_bits and acc_bits must be >= 1"
        return None
    bank = c.family in ("bank", "images")
    flat = [v for h in c.hq for v in h] if bank else list(c.hq)
    L = len(c.hq[0]) if bank else len(c.hq)
    if bank and (len(c.hq) < 1 or any(len(h) != L for h in c.hq)):
        return "filters must be >= 1"
    if c.dtype not in ("u8", "i16") or c.stage not in (U8, I32):
        return "in_dtype / out_stage"
    shapes = [(i.rows, i.width) for i in c.images] if c.family == "images" else [(c.rows, c.width)]
    if any(r < 0 or w < 0 for r, w in shapes):
        return "rows and width must be >= 0"
    if c.ch < 1:
        return "channels must be >= 1"
    if not 1 <= L <= fir_hip.MAX_TAPS or min(flat) < -(1 << 31) or max(flat) >= 1 << 31:
        return "taps"
    if c.frac < 1 or c.acc < 1:
        return "frac_bits and acc_bits must be >= 1"
    return None


# ---- strategies ------------------------------------------------------------------------------------
_FILL = st.sampled_from(["uniform", "uniform", "ends", "min", "max"])
_TYPES = [("u8", 1), ("i16", 1), ("i16", 2)]  # what the register kernel takes
_X16 = [0, 0, 16, 32, 48, 64, 256, 496]       # x leads on 16 bytes
_X8 = [8, 24, 40, 264]                        # ... on 8 but off 16 (u8: the LDS and matrix-core kernels take them)
_Y16 = [0, 0, 16, 32, 48, 256]


def _pick(draw, table):
    """An entry of the table by a hashed 32-bit key, not sampled_from: the copies hypothesis makes
    between drawn values then do not favour the first entries (0 still shrinks to the first)."""
    return table[(draw(_SEED) * 2654435761 % 2**32 * len(table)) >> 32]


def _len_edges() -> list:
    """Tap counts on both sides of every dispatch edge: 9 | 10, 39 | 40, 64 | 65 | 66, the last
    length of 3, 8, 12, 16, 24, 32 and 48 k-steps (by either count) and the first past it."""
    out = {1, 2, 3, 9, 10, 12, 13, 39, 40, 64, 65, 66, MAX_LEN}
    for ks in (_mfma_ksteps, _mfma_ksteps16):
        for k in (3, 8, 12, 16, 24, 32, 48):
            last = max(L for L in range(2, MAX_LEN + 1) if ks(L) <= k)
            out |= {last, last + 1}
    return sorted(out)


_LEN_EDGES = _len_edges()


def _length(draw, lo: int, hi: int) -> int:
    near = [e for e in _LEN_EDGES if lo <= e <= hi]
    which = draw(st.integers(0, 4))  # the edges inside the range in three draws of five, each as often as the others
    if near and which >= 2:
        return _pick(draw, near)
    return draw(st.integers(lo, hi) if which else st.integers(lo, min(hi, lo + 30)))


_RANGE = {"r24": (-(1 << 23), (1 << 23) - 1), "r16": (-32768, 32767), "mf": (-32768, 32639)}


def _values(draw, n: int, rng: str) -> list:
    """n taps inside a range, of the kinds of test_gpu_property._taps, one of them on an end of the
    range (for "r16" also 32640, the first tap past the matrix-core split) in one draw of four."""
    lo, hi = _RANGE[rng]
    kinds = ["q412", "q412", "small", "int16", "ends"] + (["mad24"] if rng == "r24" else [])
    h = np.clip(_tap_values(draw, n, kinds, -32768), lo, hi)
    if draw(st.integers(0, 3)) == 0:
        h[draw(st.integers(0, n - 1))] = draw(st.sampled_from([lo, hi] + ([32640] if rng == "r16" else [])))
    return [int(v) for v in h]


def _poke(draw, h: list, values) -> list:
    h = list(h)
    h[draw(st.integers(0, len(h) - 1))] = draw(st.sampled_from(values))
    return h


def _fit_range(L: int) -> str:
    return "r24" if L <= REG_MAX_TAPS else ("r16" if L <= LDS_MAX_TAPS else "mf")


def _past_range(L: int) -> list:
    """Taps no kernel of L taps takes."""
    if L <= REG_MAX_TAPS:
        return [1 << 23, -(1 << 23) - 1, (1 << 31) - 1, -(1 << 31)]
    return _POKE_REAL + ([32640, 32767] if L > LDS_MAX_TAPS else [])


def _frames(draw, cap: int, unit: int, edges) -> int:
    """Frames of a row: small, anywhere, whole units, or on and around an edge; at most cap."""
    edges = [e for e in edges if e >= 1]
    w = draw(st.one_of(st.integers(1, 64), st.integers(1, max(1, cap)),
                       st.integers(1, max(1, cap // unit)).map(lambda k: k * unit),
                       st.tuples(st.sampled_from(edges), st.sampled_from([-1, 0, 1, unit, -unit])).map(sum)))
    return max(1, min(w, cap))


def _row_edges(u8: bool, ch: int, L: int) -> list:
    """Where vectors, wave tiles, matrix-core tiles and workgroups end, in frames; and the shortest
    row of several the register kernel takes."""
    vec, tile = (16, 4096) if u8 else (8, 512)
    return [e // ch for e in (vec, 2 * vec, tile, 2 * tile, MF_TILE, 2 * MF_TILE, 4 * MF_TILE, 8 * MF_TILE)] + \
           [-(-(vec + (L - 1) * ch) // ch)]


def _rows_params(draw, route: str, one_row: bool = False) -> dict:
    """The drawn arguments of a rows call that takes ``route`` (one_row: a segment's bulk pass)."""
    generic = route.startswith("generic:")
    reason = route.split(":")[1] if generic else ""
    order = ("taps", "bits", "channels", "shape", "align")
    on = {reason} | {r for r in order[order.index(reason) + 1:] if draw(st.integers(0, 3)) == 0} if generic else set()
    kind = ""
    # tap count, sample type
    if route == "reg":
        L, (dtype, ch) = _length(draw, 1, 9), draw(st.sampled_from(_TYPES))
    elif route == "mfma_step":
        dtype, ch = draw(st.sampled_from(["u8", "i16"])), 1
        stage = draw(st.sampled_from([U8, I32]))
        L = _length(draw, MFMA_MIN_I32 if dtype == "i16" and stage == I32 else MFMA_MIN, 65)
    elif route in ("mfma_run", "mfma_long"):
        L, dtype, ch = _length(draw, 66, MAX_LEN), ("u8" if route == "mfma_run" else "i16"), 1
    elif route == "lds":
        kind = draw(st.sampled_from(["below40", "odd_row", "tap", "x8", "short"] if not one_row else ["below40", "odd_row", "tap", "x8"]))
        dtype, ch = draw(st.sampled_from(["u8", "i16"])), 1
        if kind == "below40":  # int16 -> int32 stays on the LDS kernel below kMfmaMinTapsI32
            L, dtype, stage = _length(draw, 10, 39), "i16", I32
        elif kind in ("odd_row", "tap"):  # one row of no multiple of 8 samples; a tap past the matrix-core split
            L = _length(draw, 10, 64)
        elif kind == "x8":  # 2-9 taps, u8 x at 8 mod 16: off the register kernel, on the LDS kernel
            L, dtype = _length(draw, 2, 9), "u8"
        else:  # 2-9 taps, several rows of 8 (u8: or 16) samples: shorter than a vector plus the halo
            L = _length(draw, 2, 9)
    else:
        # the tap counts of the register kernel, of the LDS kernel, and past it (one row has a shape
        # no kernel takes only there)
        lo, hi = draw(st.sampled_from([(1, 9), (10, 64), (65, MAX_LEN)] if not (one_row and reason == "shape") else [(65, MAX_LEN)]))
        L = _length(draw, lo, hi)
        if "channels" in on:
            dtype, ch = draw(st.sampled_from([("u8", 2), ("u8", 3), ("i16", 3)] + ([("i16", 2)] if L > 9 else [])))
        else:
            dtype, ch = draw(st.sampled_from(_TYPES if L <= 9 else _TYPES[:2]))
    if route != "mfma_step" and kind != "below40":
        stage = draw(st.sampled_from([U8, I32]))
    u8 = dtype == "u8"
    # taps
    if generic:
        hq = _values(draw, L, _fit_range(L))
        if "taps" in on:
            hq = _poke(draw, hq, _past_range(L))
    elif route == "reg":
        hq = _values(draw, L, "r24")
    elif route == "lds":
        hq = _values(draw, L, "r16")
        if kind == "tap":
            hq = _poke(draw, hq, [32640, 32767, 32700])
    else:
        hq = _values(draw, L, "mf")
    frac, acc = _bits(draw, {"bits"} if "bits" in on else set())
    # rows and width
    rows = 1 if one_row else draw(st.one_of(st.just(1), st.integers(2, 40)))
    if kind == "odd_row":
        rows = 1
    if kind == "short" or ("shape" in on and L <= LDS_MAX_TAPS):
        rows = 1 if one_row else draw(st.integers(2, 40))
    cap = max(1, min(33000 if u8 else 8400, WORK // (rows * ch * L)))
    w = _frames(draw, cap, 8 // math.gcd(8, ch), _row_edges(u8, ch, L))
    vec = 16 if u8 else 8
    need = -(-(vec + (L - 1) * ch) // ch)  # frames of the shortest row of several on the register kernel
    if kind == "short":
        w = 8 if not u8 else draw(st.sampled_from([8, 16]))
    elif "shape" in on:
        if L <= REG_MAX_TAPS:  # shorter than a vector plus the halo, and no row of whole LDS vectors
            w = draw(st.one_of(st.just(need - 1), st.integers(1, need - 1)))
            if ch == 1 and L >= 2 and w % 8 == 0:
                w -= 1
        elif (w * ch) % 8 == 0:
            w += 1
    elif route == "reg" or (generic and L <= REG_MAX_TAPS):
        if rows > 1:
            w = max(w, need)
    elif route in ("mfma_step", "mfma_run", "mfma_long") or (generic and L > LDS_MAX_TAPS):
        w = max(8, w // 8 * 8) if ch == 1 else w  # rows (or the one row) of whole 8-sample vectors
    elif kind == "odd_row":
        w += w % 8 == 0
    elif rows > 1 and ch == 1:  # the LDS kernel's rows, and the generic calls of 10-64 taps
        w = max(8, w // 8 * 8)
    # leads
    ysz = 4 if stage == I32 else 1
    if "align" in on:
        which = draw(st.sampled_from(["x", "y", "xy"]))
        bad_x = [1, 2, 3, 4, 5, 6, 7, 9, 12, 20] if u8 else [2, 4, 6, 8, 10, 12, 14, 18, 24, 40]
        x_lead = draw(st.sampled_from(bad_x if "x" in which else _X16))
        y_lead = draw(st.sampled_from([1, 2, 3, 5, 6, 7, 9])) * ysz if "y" in which else draw(st.sampled_from(_Y16))
    else:  # u8 past 9 taps: 8 mod 16 suits every kernel the call can take
        x_lead = draw(st.sampled_from(_X8 if kind == "x8" else _X16 + (_X8 if u8 and L > REG_MAX_TAPS else [])))
        y_lead = draw(st.sampled_from(_Y16))
    return dict(dtype=dtype, ch=ch, stage=stage, hq=tuple(hq), frac=frac, acc=acc, rows=rows, width=w, x_lead=x_lead,
                y_lead=y_lead)


@st.composite
def rows_case(draw):
    route = _pick(draw, ROUTES["rows"])
    return Case("rows", route, seed=draw(_SEED), fill=draw(_FILL), **_rows_params(draw, route))


@st.composite
def segment_case(draw):
    route = _pick(draw, ["one", "rows+edges", "rows+edges", "all_edge"])
    halos = (draw(st.booleans()), draw(st.booleans()))
    if route == "one":
        p = _rows_params(draw, "reg", one_row=True)
        tile = (4096 if p["dtype"] == "u8" else 512) // p["ch"]
        p["width"] = draw(st.sampled_from([1, 1, 2, 3, 4])) * tile
    elif route == "rows+edges":
        sub = _pick(draw, ROUTES["rows"])
        p = _rows_params(draw, sub, one_row=True)
        u8, ch, L = p["dtype"] == "u8", p["ch"], len(p["hq"])
        # longer than its halos, without leaving the bulk pass's own kernel: whole 8-sample vectors
        # stay whole, a ragged row stays ragged
        if p["width"] * ch <= (L - 1) * ch:
            p["width"] = (L + 7) // 8 * 8 + (p["width"] * ch % 8 != 0)
        tile = (4096 if u8 else 512) // ch
        if sub == "reg" and draw(st.integers(0, 2)) == 0:  # one frame off a whole number of wave tiles
            p["width"] = draw(st.sampled_from([1, 1, 2, 3])) * tile + draw(st.sampled_from([-1, 1]))
        if sub == "reg" and p["width"] % tile == 0:  # whole wave tiles would be one launch
            p["width"] += 1
    else:
        p = _rows_params(draw, _pick(draw, ["reg", "reg", "lds", "generic:taps", "generic:bits", "generic:channels", "generic:align",
                                            "mfma_step", "mfma_run", "mfma_long"]), one_row=True)
        L = len(p["hq"])
        if L == 1:  # one tap has no halo: give it two
            p["hq"] = p["hq"] + (draw(st.integers(-8192, 8192)),)
            L = 2
        p["width"] = draw(st.one_of(st.just(1), st.just(L - 1), st.integers(1, L - 1)))
    lead = st.sampled_from([0, 0, 2, 6, 8, 16, 30, 254] + ([1, 3, 7] if p["dtype"] == "u8" else []))  # a halo lies at any element
    return Case("segment", route, seed=draw(_SEED), fill=draw(_FILL), halos=halos, hl_lead=draw(lead), hr_lead=draw(lead), **p)


def _bank_taps(draw, F: int, L: int, rng: str, seeded: bool = False) -> list:
    """F filters of L taps, drawn as one tap set (past 32 taps, or when ``seeded``, from a seed:
    cheap to draw)."""
    flat = _values(draw, max(F * L, 33 if seeded else 0), rng)
    return [flat[f * L:(f + 1) * L] for f in range(F)]


@st.composite
def bank_case(draw):
    route = _pick(draw, ROUTES["bank"])
    F = draw(st.one_of(st.integers(1, 8), st.sampled_from([1, 4, 5, 8])))
    stage = draw(st.sampled_from([U8, I32]))
    why = "" if route == "fused" else draw(st.sampled_from(["type", "taps10", "bits", "tap", "x", "y", "short"]))
    dtype, ch = ("u8", 1) if why != "type" else draw(st.sampled_from([("i16", 1), ("i16", 2), ("u8", 2), ("u8", 3), ("i16", 3)]))
    L = _length(draw, 10, 70) if why == "taps10" else _length(draw, 1, 9)
    hq = _bank_taps(draw, F, L, "r24" if L <= 9 else "r16")
    if why == "tap":
        f = draw(st.integers(0, F - 1))
        hq[f] = _poke(draw, hq[f], _past_range(L))
    frac, acc = _bits(draw, {"bits"} if why == "bits" else set())
    rows = draw(st.integers(2, 30)) if why == "short" else draw(st.one_of(st.just(1), st.integers(2, 30)))
    u8 = dtype == "u8"
    cap = max(1, min(9000 if u8 else 2100, WORK // (F * rows * ch * L)))
    w = _frames(draw, cap, 8 // math.gcd(8, ch), _row_edges(u8, ch, L) + [640, 1280, 4499])
    need = -(-((16 if u8 else 8) + (L - 1) * ch) // ch)
    if why == "short":
        w = draw(st.integers(1, need - 1))
    elif rows > 1 and L <= 9:
        w = max(w, need)
    x_lead = draw(st.sampled_from([1, 3, 4, 8, 12, 24] if why == "x" else _X16))
    if why == "y":  # int32 planes off 16 bytes: by plane 0's address, or by planes of no whole 16 bytes
        stage = I32
        if draw(st.booleans()):
            y_lead = draw(st.sampled_from([4, 8, 12, 20, 36]))
        else:
            y_lead, rows, w = draw(st.sampled_from(_Y16)), rows | 1, w | 1
    elif stage == U8:
        y_lead = draw(st.one_of(st.sampled_from(_Y16), st.integers(0, 15), st.sampled_from([1, 7, 8, 13, 509])))
    else:
        y_lead = draw(st.sampled_from(_Y16))
        if route == "fused":  # the int32 planes of a fused bank are whole 16 bytes
            w = (w + 3) // 4 * 4
    return Case("bank", route, dtype, ch, stage, tuple(tuple(h) for h in hq), frac, acc, rows, w, seed=draw(_SEED),
                fill=draw(_FILL), x_lead=x_lead, y_lead=y_lead)


@st.composite
def images_case(draw):
    route = _pick(draw, ROUTES["images"])
    n = _pick(draw, [0, 1, 1, 2, 2, 3, 3, 4] * 3 + [5, 6, 7, 8, 8, 9, 9, 10, 12, 16, 17, 20])  # two cases of three hold at most 4
    why = draw(st.sampled_from(["type", "stage", "taps10", "bits", "tap", "image"])) if route == "single" else ""
    if route == "mixed" or why == "image":
        n = max(n, 2 if route == "mixed" else 1)
    # every plane is a guarded allocation of its own, so a case holds at most 16 of them (by min()), one
    # case of twelve up to 48: only those meet several launches of more than four filters
    planes = 48 if draw(st.integers(0, 11)) == 0 else 16
    F = min(draw(st.one_of(st.integers(1, 8), st.sampled_from([1, 4, 5, 8]))), max(1, planes // max(n, 1)))
    dtype, ch = draw(st.sampled_from([("i16", 1), ("i16", 2), ("i16", 3), ("u8", 2)])) if why == "type" else ("u8", 1)
    stage = I32 if why == "stage" else (U8 if why != "type" else draw(st.sampled_from([U8, I32])))
    L = draw(st.integers(10, 12)) if why == "taps10" else draw(st.one_of(st.integers(1, 9), st.sampled_from([1, 3, 5, 9])))
    hq = _bank_taps(draw, F, L, "r24" if L <= 9 else "r16", seeded=F > 1)
    if why == "tap":
        f = draw(st.integers(0, F - 1))
        hq[f] = _poke(draw, hq[f], _past_range(L))
    frac, acc = _bits(draw, {"bits"} if why == "bits" else set())
    u8, ysz = dtype == "u8", 4 if stage == I32 else 1
    eligible = route != "single" or why == "image"  # the call's filters and types allow the batch kernel
    need = 16 + L - 1
    cap = max(32, min(5000, WORK // (max(n, 1) * F * 12 * ch * L)))
    images = []
    for i in range(n):
        if not eligible:
            kind = draw(st.sampled_from(["plain", "plain", "onerow", "empty", "narrow", "off16"]))
        elif route == "batch":
            kind = draw(st.sampled_from(["plain", "plain", "whole", "onerow", "empty"]))
        elif route == "single":
            kind = draw(st.sampled_from(["narrow", "off16"] + (["empty"] if i else [])))
        else:  # mixed: image 0 on the batch kernel, image 1 off it
            kind = ["plain", "off16"][i] if i < 2 else draw(st.sampled_from(["plain", "whole", "onerow", "empty", "narrow", "off16"]))
        # the image's sizes and leads from one seed (an image list drawn value by value costs more
        # than the calls it makes): rows 1-12, a width that is small, anywhere, or on and around a
        # vector, a wave tile or the 1024-sample tile of a bank; every plane at a lead of its own, on 16
        # bytes, at any element (u8 planes: any byte) or on a cache line
        rng = np.random.default_rng(draw(_SEED))
        pick = lambda seq: seq[int(rng.integers(0, len(seq)))]  # noqa: E731
        rows = 1 if kind == "onerow" else int(rng.integers(2 if kind == "narrow" else 1, 13))
        if kind == "narrow":  # several rows shorter than a vector plus the halo
            w = int(rng.integers(1, max(1, (need - 1) // ch) + 1))
        elif kind == "whole":  # whole 16-byte vectors: no seam to patch
            w = 16 * int(rng.integers(-(-need // 16), max(-(-need // 16), cap // 16) + 1))
        else:  # one row may be narrower than the register kernel's minimum
            w = pick([int(rng.integers(1, 65)), int(rng.integers(1, cap + 1)),
                      pick([16, 64, 1024, 1040, 4096]) + pick([-1, 0, 1, 16, -16])])
            w = max(1, min(w, cap)) if rows == 1 else max(-(-need // ch), min(w, cap))
        if kind == "empty":
            rows, w = pick([(0, w), (rows, 0), (0, 0)])
        x_lead = pick(([1, 2, 3, 4, 8, 9, 24] if u8 else [2, 4, 8, 12, 24]) if kind == "off16" else _X16)
        table = _Y16 + [k * ysz for k in range(16)] * 2 + [128, 384]
        y_leads = tuple(table[k] for k in rng.integers(0, len(table), F))
        images.append(Image(rows, w, x_lead, y_leads))
    return Case("images", route, dtype, ch, stage, tuple(tuple(h) for h in hq), frac, acc, seed=draw(_SEED), fill=draw(_FILL),
                images=tuple(images))


def _taps2d(draw, R: int, C: int, kind: str) -> np.ndarray:
    """The tap kinds of test_gpu_property.fir2d_case and fir2d_mfma_case."""
    if kind == "outer":  # exactly rank-1
        col = draw(st.lists(st.integers(-64, 64), min_size=R, max_size=R))
        row = draw(st.lists(st.integers(-64, 64), min_size=C, max_size=C))
        return np.outer(col, row) * draw(st.sampled_from([1, 4, 16]))
    lim = {"small": 8, "q412": 4096, "wide": 1 << 20, "byte": 127, "pow2": 127, "pair": 8192, "pair_wide": 32639, "int16": 32767}[kind]
    h = np.asarray(draw(st.lists(st.integers(-lim - (kind != "wide"), lim), min_size=R * C, max_size=R * C)), dtype=np.int64).reshape(R, C)
    return h * (1 << draw(st.integers(1, 10))) if kind == "pow2" else h


@st.composite
def fir2d_case(draw):
    route = _pick(draw, ROUTES["fir2d"])
    path, stage, bad = draw(st.sampled_from([None, None, "reg", "mfma"])), U8, ""
    frac = draw(st.one_of(st.just(12), st.integers(1, 24)))
    acc = draw(st.one_of(st.just(32), st.integers(max(12, frac - 4), 32)))
    odd135 = st.sampled_from([1, 3, 5])
    if route == "mfma":
        R, C = draw(st.sampled_from([3, 5])), draw(st.integers(1, 5))
        # every tap inside the balanced byte pair, whatever power of two the plan takes out
        h = np.clip(_taps2d(draw, R, C, draw(st.sampled_from(["byte", "byte", "pow2", "pair", "pair_wide", "outer"]))), -32768, 32639)
        if path == "reg" or (path is None and sep2d_register_form(h.tolist())):
            path = "mfma"  # a rank-1 kernel of a register shape takes the matrix cores only when forced
    elif route == "pk16_strip":
        R, C, path = draw(st.sampled_from([3, 5])), draw(st.sampled_from([3, 5])), draw(st.sampled_from([None, "reg"]))
        signed = draw(st.booleans())  # factors in [-2, 2] (signed 16-bit sums) or [0, 3] (unsigned)
        each = st.integers(-2, 2) if signed else st.integers(0, 3)
        col, row = draw(st.lists(each, min_size=R, max_size=R)), draw(st.lists(each, min_size=C, max_size=C))
        col[R // 2], row[C // 2] = col[R // 2] or 1, row[C // 2] or 2  # neither factor is all zero
        k = draw(st.integers(0, 6))
        h = np.outer(col, row) * (1 << k)
        frac = draw(st.integers(k + 1, 13 + k))  # the plan takes 2^k out and keeps at most 13 bits of rounding half
        acc = draw(st.one_of(st.just(32), st.integers(24, 32)))
    elif route == "reg":
        kind = draw(st.sampled_from(["i32", "line", "row1", "sep_wide", "split"]))
        R, C = draw(odd135), draw(odd135)
        if kind == "i32":  # the int32 stage: neither matrix cores nor packed 16
            stage, h = I32, np.clip(_taps2d(draw, R, C, draw(st.sampled_from(["outer", "small", "q412", "int16"]))), -32768, 32767)
        elif kind == "line":  # one tap row or column on the register path: never separable
            path = "reg"
            R, C = draw(st.sampled_from([(1, C), (R, 1)]))
            h = _taps2d(draw, R, C, draw(st.sampled_from(["small", "q412", "int16"])))
        elif kind == "row1":  # one tap row: no matrix-core form
            R, path = 1, draw(st.sampled_from([None, "reg", "mfma"]))
            h = _taps2d(draw, R, C, draw(st.sampled_from(["small", "q412", "int16"])))
        elif kind == "sep_wide":  # rank-1 with odd factors and 16 or more fraction bits: no packed-16 plan
            R, C, path = draw(st.sampled_from([3, 5])), draw(st.sampled_from([3, 5])), draw(st.sampled_from([None, "reg"]))
            odd = st.integers(-20, 20).map(lambda v: 2 * v + 1)
            h = np.outer(draw(st.lists(odd, min_size=R, max_size=R)), draw(st.lists(odd, min_size=C, max_size=C)))
            frac = draw(st.integers(16, 31))
            acc = draw(st.one_of(st.just(32), st.integers(frac - 4, 32)))
        else:  # an odd tap past the balanced byte pair: the matrix-core plan refuses, the register path does not
            R, path = draw(st.sampled_from([3, 5])), draw(st.sampled_from([None, "reg", "mfma"]))
            h = _taps2d(draw, R, C, "q412")
            h[R - 1, C - 1] = draw(st.sampled_from([32641, 32767, 32765]))
            h[0, 0] |= 1  # an odd tap: no common power of two to take out
            if C > 1:
                h[0, 1], h[1, 0], h[1, 1] = 0, 0, 1  # ... and not rank-1 (h[0, 0] is odd, so not zero)
    else:
        bad = draw(st.sampled_from(["width", "align", "bits", "tap", "shape", "shape_i32"]))
        R, C = draw(st.integers(1, 7)), draw(st.integers(1, 7))
        stage = draw(st.sampled_from([U8, U8, I32]))
        if bad == "shape":  # no kernel of either path for these tap shapes
            R, C = draw(st.sampled_from([(2, C), (4, C), (6, C), (7, C), (1, 2), (1, 4), (1, 6), (1, 7), (3, 6), (5, 7)]))
        elif bad == "shape_i32":  # the matrix cores would take them, the stage or the path does not
            R, C = draw(st.sampled_from([3, 5])), draw(st.sampled_from([2, 4]))
            stage, path = draw(st.sampled_from([(I32, path), (U8, "reg")]))
        h = _taps2d(draw, R, C, draw(st.sampled_from(["outer", "small", "q412", "wide" if bad == "tap" else "int16"])))
        if bad == "tap":
            odd_past_int16 = st.sampled_from([32769, -32769, (1 << 20) + 1, (1 << 31) - 1])
            h[draw(st.integers(0, R - 1)), draw(st.integers(0, C - 1))] = draw(odd_past_int16)
        if bad == "bits":
            frac, acc = _bits(draw, {"bits"})
    frames = draw(st.sampled_from([0, 0, 1, 2, 3]))
    H = draw(st.one_of(st.integers(1, 40), st.integers(41, 300), st.sampled_from([15, 16, 17, 32, 33])))
    cap = max(16, min(1100, WORK // (max(frames, 1) * H * R * C)))
    W = draw(st.one_of(st.integers(1, 80), st.integers(1, 1100), st.integers(1, 68).map(lambda k: 16 * k),
                       st.integers(1024 - 16, 1024 + 16), st.sampled_from([1008, 1024, 1040])))
    W = min(W, cap)
    if bad == "width":
        W += W % 16 == 0
    else:
        W = max(16, W // 16 * 16)
    x_lead = draw(st.sampled_from([1, 3, 4, 8, 12, 24] if bad == "align" and draw(st.booleans()) else _X16))
    ysz = 4 if stage == I32 else 1
    y_lead = draw(st.sampled_from([1, 2, 3, 5, 7])) * ysz if bad == "align" and (x_lead % 16 == 0 or draw(st.booleans())) \
        else draw(st.sampled_from(_Y16))
    return Case("fir2d", route, stage=stage, hq=tuple(tuple(int(v) for v in r) for r in h), frac=frac, acc=acc, rows=H, width=W,
                frames=frames, seed=draw(_SEED), fill=draw(_FILL), x_lead=x_lead, y_lead=y_lead, path=path)


_IDEAL_TAP = st.one_of(st.floats(-8.0, 8.0, allow_nan=False, allow_infinity=False), st.sampled_from([0.25, 0.5, -1.0, 1 / 3, 0.0, -0.0]))


@st.composite
def ideal_case(draw):
    route = _pick(draw, ROUTES["ideal"])
    reg = route.endswith("reg")
    bad = "" if reg else draw(st.sampled_from(["taps", "x", "y", "shape"]))
    x_lead = draw(st.sampled_from([1, 2, 3, 5, 6, 7, 9] if bad == "x" else [0, 0, 4, 8, 12, 16, 36, 256]))
    y_lead = draw(st.sampled_from([8, 24, 40, 264] if bad == "y" else _Y16))
    if route.startswith("1d"):
        L = draw(st.integers(10, 40) if bad == "taps" else st.integers(1, 9))
        rows = draw(st.integers(2, 20)) if bad == "shape" else draw(st.one_of(st.just(1), st.integers(2, 20)))
        w = _frames(draw, max(1, min(9000, WORK // (rows * L))), 4, [4, 256, 1024, 2048, 4 + L - 1])
        if bad == "shape":  # several rows shorter than a dword plus the halo
            w = draw(st.integers(1, 4 + L - 2))
        elif rows > 1 and bad != "taps":
            w = max(w, 4 + L - 1)
        hq, frames = tuple(draw(st.lists(_IDEAL_TAP, min_size=L, max_size=L))), 0
    else:
        R, C = (draw(st.integers(1, 5)), draw(st.integers(1, 5))) if bad != "taps" else \
            draw(st.sampled_from([(6, 3), (3, 6), (7, 7), (1, 6), (6, 1)]))
        frames = draw(st.sampled_from([0, 0, 1, 2, 3]))
        rows = draw(st.one_of(st.integers(1, 40), st.sampled_from([15, 16, 17, 33])))
        w = _frames(draw, max(8, min(2100, WORK // (max(frames, 1) * rows * R * C))), 4, [4, 8, 1024, 2048])
        if bad == "shape":  # no whole dwords, or narrower than a dword plus the halo
            w = w + (w % 4 == 0) if draw(st.booleans()) or C == 1 else draw(st.integers(1, 4 + C - 2))
        else:
            w = max(8, w // 4 * 4)
        flat = draw(st.lists(_IDEAL_TAP, min_size=R * C, max_size=R * C))
        hq = tuple(tuple(flat[m * C:(m + 1) * C]) for m in range(R))
    return Case("ideal", route, hq=hq, rows=rows, width=w, frames=frames, seed=draw(_SEED), fill=draw(_FILL), x_lead=x_lead,
                y_lead=y_lead)


STRATEGIES = {"rows": rows_case, "bank": bank_case, "images": images_case, "segment": segment_case, "fir2d": fir2d_case,
              "ideal": ideal_case}


# ---- pinned examples: the thresholds a random draw reaches rarely, every route at least once -------------
def _ramp(n, lo=-2000, step=37):
    return tuple(lo + step * k for k in range(n))


def _with(h, k, v):
    return h[:k] + (v,) + h[k + 1:]


def _low(n):  # taps of a long low-pass: small, so no sum wraps 32 bits
    return tuple(((k * 7919) % 41) - 20 for k in range(n))


_SEP3 = tuple(tuple(a * b for b in (65, 127, 65)) for a in (63, 129, 63))  # rank-1, odd factors, sum 2^16 - 1
_H9, _BANK = _ramp(9), (_ramp(5, -300, 150), _ramp(5, 900, -210), (0, 0, 4096, 0, 0), _ramp(5, -1, 1), (1, 2, 3, 2, 1))
TALL = [
    # the tallest frame the 2-D register kernel takes (gridDim.y = 65535), and the first past it; 16
    # fraction bits over odd taps leave no packed-16 plan, so the separable register kernel itself runs
    Case("fir2d", "reg", hq=_SEP3, frac=16, rows=TALL_H, width=16, seed=7),
    Case("fir2d", "generic", hq=_SEP3, frac=16, rows=TALL_H + 1, width=16, seed=7),
]
PINNED = {
    "rows": [
        Case("rows", "reg", "u8", hq=_H9, rows=3, width=24), Case("rows", "generic:shape", "u8", hq=_H9, rows=3, width=23),
        Case("rows", "lds", "u8", hq=_H9, rows=3, width=16),
        Case("rows", "reg", "i16", 2, I32, _H9, rows=2, width=12),
        Case("rows", "generic:shape", "i16", 2, I32, _H9, rows=2, width=11),
        Case("rows", "reg", "i16", 1, I32, _with(_H9, 4, (1 << 23) - 1), width=520),
        Case("rows", "generic:taps", "i16", 1, I32, _with(_H9, 4, 1 << 23), width=520),
        Case("rows", "lds", "i16", 1, I32, _ramp(10), width=1032), Case("rows", "mfma_step", "i16", 1, U8, _ramp(10), width=1032),
        Case("rows", "lds", "i16", 1, I32, _ramp(39), width=1032), Case("rows", "mfma_step", "i16", 1, I32, _ramp(40), width=1032),
        Case("rows", "mfma_step", "u8", hq=_low(65), rows=2, width=2056),
        Case("rows", "mfma_run", "u8", hq=_low(66), rows=2, width=2056),
        Case("rows", "mfma_step", "i16", 1, I32, _low(65), width=1032),
        Case("rows", "mfma_long", "i16", 1, I32, _low(66), width=1032),
        Case("rows", "lds", "u8", hq=_with(_low(64), 3, 32640), width=1032),
        Case("rows", "generic:taps", "u8", hq=_with(_low(65), 3, 32640), width=1032),
        Case("rows", "mfma_step", "u8", hq=_with(_low(64), 3, 32639), width=1032),
        Case("rows", "mfma_run", "u8", hq=_low(1000), width=2048), Case("rows", "mfma_run", "u8", I32, hq=_low(1500), width=2048),
        Case("rows", "mfma_long", "i16", 1, U8, _low(1500), width=2048),
        Case("rows", "mfma_long", "i16", 1, I32, _low(MAX_LEN), width=1024),
        Case("rows", "lds", "u8", hq=_ramp(16), width=1031), Case("rows", "generic:shape", "u8", hq=_low(70), width=1031),
        Case("rows", "generic:bits", "u8", hq=_H9, acc=33, width=264, fill="ends"),
        Case("rows", "generic:bits", "i16", hq=_ramp(16), frac=32, width=264),
        Case("rows", "generic:channels", "u8", 2, hq=_H9, width=260),
        Case("rows", "generic:channels", "i16", 3, I32, _H9, rows=2, width=100),
        Case("rows", "generic:channels", "i16", 2, I32, _ramp(16), width=260),
        Case("rows", "lds", "u8", hq=_H9, rows=2, width=264, x_lead=8),
        Case("rows", "generic:align", "i16", 1, I32, _H9, rows=2, width=264, x_lead=8),
        Case("rows", "generic:align", "u8", hq=_H9, rows=2, width=264, y_lead=1),
        Case("rows", "mfma_step", "u8", hq=_ramp(16), width=264, x_lead=8),
    ],
    "bank": [
        Case("bank", "fused", hq=_BANK, rows=3, width=4499, y_lead=1),
        Case("bank", "fused", stage=I32, hq=_BANK[:4], rows=4, width=21),
        Case("bank", "each", stage=I32, hq=_BANK[:2], rows=3, width=21),
        Case("bank", "each", stage=I32, hq=_BANK[:2], rows=4, width=21, y_lead=8),
        Case("bank", "each", hq=_BANK[:3], rows=2, width=264, x_lead=8),
        Case("bank", "each", "i16", 2, I32, _BANK[:3], rows=2, width=132),
        Case("bank", "each", hq=(_ramp(16), _ramp(16, 5, -3)), rows=2, width=1032, y_lead=16),
    ],
    "images": [
        Case("images", "batch", hq=_BANK, images=tuple(
            Image(r, w, 0, tuple(range(f, f + 5)))
            for f, (r, w) in enumerate([(3, 40), (1, 5), (0, 7), (2, 4099), (5, 64), (4, 21), (1, 1), (2, 33), (7, 20)]))),
        Case("images", "single", stage=I32, hq=_BANK[:2], images=(Image(3, 40, 0, (0, 16)), Image(1, 5, 16, (4, 32)))),
        Case("images", "single", "i16", hq=_BANK[:1], images=(Image(3, 40, 0, (2,)),)),
        Case("images", "single", hq=(_ramp(10),), images=(Image(3, 40, 0, (0,)), Image(2, 64, 8, (16,)))),
        Case("images", "mixed", hq=_BANK[:2],
             images=(Image(3, 40, 0, (3, 5)), Image(3, 19, 0, (0, 16)), Image(2, 64, 8, (0, 7)), Image(1, 9, 0, (1, 1)))),
        Case("images", "batch", hq=_BANK[:1], images=()),
    ],
    "segment": [
        Case("segment", "one", "u8", hq=_H9, width=4096), Case("segment", "rows+edges", "u8", hq=_H9, width=4097),
        Case("segment", "rows+edges", "u8", hq=_H9, width=4096, x_lead=8),
        Case("segment", "one", "i16", 2, I32, _H9, width=512, halos=(True, False)),
        Case("segment", "rows+edges", "i16", 1, I32, _low(300), width=1024, halos=(False, True), hl_lead=2, hr_lead=6),
        Case("segment", "rows+edges", "u8", hq=_low(300), width=304), Case("segment", "rows+edges", "u8", hq=_ramp(16), width=300),
        Case("segment", "rows+edges", "u8", hq=(4096,), width=300),
        Case("segment", "all_edge", "u8", hq=_low(300), width=299, hr_lead=3),
        Case("segment", "all_edge", "i16", 2, I32, _H9, width=8),
        Case("segment", "all_edge", "i16", 3, I32, _H9, width=1, halos=(False, False)),
    ],
    "fir2d": TALL + [
        Case("fir2d", "pk16_strip", hq=((1, 2, 1), (2, 4, 2), (1, 2, 1)), frac=4, rows=33, width=1040, frames=2),
        Case("fir2d", "mfma", hq=((1, 2, 1), (2, 4, 2), (1, 2, 1)), frac=4, rows=33, width=1040, frames=2, path="mfma"),
        Case("fir2d", "reg", hq=((1, 2, 1), (2, 4, 2), (1, 2, 1)), frac=4, rows=33, width=1040, stage=I32),
        Case("fir2d", "mfma", hq=((0, -1024, 0), (-1024, 8192, -1024), (0, -1024, 0)), rows=17, width=64),
        Case("fir2d", "reg", hq=((0, -1024, 0), (-1024, 8192, -1024), (0, -1024, 0)), rows=17, width=64, path="reg"),
        Case("fir2d", "generic", hq=((0, -1024, 0), (-1024, 8192, -1024), (0, -1024, 0)), rows=17, width=63),
        Case("fir2d", "generic", hq=((0, -1024, 0), (-1024, 8192, -1024), (0, -1024, 0)), rows=17, width=64, y_lead=8),
        Case("fir2d", "generic", hq=((1, 2), (3, 4)), frac=3, rows=9, width=32),
    ],
    "ideal": [
        Case("ideal", "1d:reg", hq=(0.25, 0.5, 0.25), rows=3, width=6),
        Case("ideal", "1d:generic", hq=(0.25, 0.5, 0.25), rows=3, width=5),
        Case("ideal", "1d:reg", hq=tuple(0.1 * k for k in range(9)), width=1031, x_lead=4),
        Case("ideal", "1d:generic", hq=tuple(0.1 * k for k in range(10)), width=1031),
        Case("ideal", "1d:generic", hq=(0.5, 0.5), width=64, x_lead=2),
        Case("ideal", "1d:generic", hq=(0.5, 0.5), width=64, y_lead=8),
        Case("ideal", "2d:reg", hq=((0.0, 0.25, 0.0), (0.25, -1.0, 0.25), (0.0, 0.25, 0.0)), rows=17, width=8, frames=2),
        Case("ideal", "2d:generic", hq=((0.0, 0.25, 0.0), (0.25, -1.0, 0.25), (0.0, 0.25, 0.0)), rows=17, width=5),
        Case("ideal", "2d:generic", hq=((0.5,) * 6,), rows=4, width=16),
        Case("ideal", "2d:generic", hq=((0.5,),), rows=4, width=16, x_lead=2),
    ],
}


def pinned_for_hypothesis(fam: str) -> list:
    """PINNED without the two tall frames, which have a test (and a time) of their own."""
    return [c for c in PINNED[fam] if c not in TALL]


def smaller(c: Case, rows: int = 2, width: int = 11, taps: int = 5) -> Case:
    """The case cut down to a few taps, rows and frames (its route no longer matters): for the CPU
    test that holds ``want`` against a direct loop over the definition."""
    if c.family in ("bank", "images"):
        c = replace(c, hq=tuple(h[:taps] for h in c.hq[:3]))
        if c.family == "images":
            return replace(c, images=tuple(Image(min(i.rows, rows), min(i.width, width), i.x_lead, i.y_leads[:3]) for i in c.images[:4]))
        return replace(c, rows=min(c.rows, rows), width=min(c.width, width))
    return replace(c, hq=c.hq[:taps], rows=min(c.rows, rows), width=min(c.width, width))
