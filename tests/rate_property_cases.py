"""Hypothesis strategies, dispatch restatements and references for the four rate-changing / complex
FIR families -- a test helper, not a test module.

tests/test_gpu_property_rate.py runs the strategies on the GPU; tests/test_rate_property_cases.py
keeps this module honest without one.  The families and their entries:

    decim     torch_ops.fir1d_fixed_rows_decim_dev            csrc/fir1d_decim.hip
    interp    torch_interp.fir1d_fixed_rows_interp_dev        csrc/fir1d_interp.hip
    resample  torch_resample.fir1d_fixed_rows_resample_dev    csrc/fir1d_resample.hip
    cplx      torch_cplx.fir1d_fixed_rows_cplx_dev            csrc/fir1d_cplx.hip

References (nothing new: the grids' own, stated once here and imported by test_gpu_decim.py,
test_gpu_interp.py and test_gpu_resample.py): the committed C oracle at full rate, on the NumPy
zero-stuffed signal where the family stuffs, sliced [:, phase::D] where it decimates; the complex
family's is tests/cplx_ref.py's ``want``.  Every comparison is np.array_equal.

Routes, by construction.  A strategy first draws the route it intends and then builds a call that
takes it: no assume(), no .filter().  A call is off the fast kernel for one or more REASONS, which
``route_of`` checks in one fixed order (forward, rate, taps, bits, stage, shape, align) and names by
the first that holds.  A strategy that intends ``generic:X`` switches X on, every reason before X
off, and each reason after X on in about one draw of four, so the generic kernels also meet
combinations (three channels at U = 17 with a row shorter than D) and ``route_of`` still has one
answer.  ``forward`` draws every reason freely: the call it is forwarded to may take any kernel.

    fast            the LDS polyphase / sliding-window v_dot2 kernel
    generic:rate    U or D of 1 (decimator, interpolator) or above 16
    generic:taps    too many taps, or a tap outside int16 (complex: outside [-32767, 32767])
    generic:bits    acc_bits > 32 or frac_bits > 31
    generic:stage   the u8 stage (complex only)
    generic:shape   several rows of a length that is no multiple of 8 samples (complex: 4 frames),
                    three channels, u8 of two channels
    generic:align   x off 16 bytes (u8: 8); complex: y off 16 bytes too
    forward         resampler: up == 1 or decim == 1; complex: every hi == 0

Sizes.  A reference costs rows * width * channels * U * L multiply-adds on the host, so a drawn
width is capped at WORK of them (by min(), not by rejection): the longest filters (1024 taps at
U = 16) meet rows of a pass or two, every filter up to a few hundred taps meets rows past two
workgroups.  The grids hold the longest filters on the workgroup edges.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
from hypothesis import strategies as st

import fir_hip
from cplx_ref import want as cplx_want
from oracle import c_oracle

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32
FAMILIES = ("decim", "interp", "resample", "cplx")

# The limits of the fast kernels, as the sources state them (tests/test_rate_property_cases.py
# reads the constants back from the files named here).
LIMITS = {
    "kDecMaxD": ("fir1d_decim.hip", 16), "kDecMaxTaps": ("fir1d_decim.hip", 128),
    "kIntMaxU": ("fir1d_interp.hip", 16), "kIntMaxTaps": ("fir1d_interp.hip", 128),
    "kResMaxUD": ("fir1d_resample.hip", 16), "kResMaxPhaseTaps": ("fir1d_resample.hip", 64),
    "kCxMaxTaps": ("fir1d_cplx.hip", 64), "kCxVec": ("fir1d_cplx.hip", 4),
}
MAX_RATE = 16        # kDecMaxD, kIntMaxU, kResMaxUD
MAX_TAPS_REAL = 128  # kDecMaxTaps, kIntMaxTaps
MAX_PHASE_TAPS = 64  # kResMaxPhaseTaps: ceil(L / U)
MAX_TAPS_CPLX = 64   # kCxMaxTaps
CPLX_VEC = 4         # kCxVec
TOP_RATE = 40        # the largest U or D drawn
LONG_TAPS = 400      # "a few hundred": the longest drawn filter past a limit (the resampler's limit, 64 U, is longer)
# input frames a drawn row may have: just past two workgroups of the family where the reference's cost allows
MAX_WIDTH = {"decim": 9000, "interp": 4500, "resample": 4500, "cplx": 2100}
WORK = 3 * 10**7     # multiply-adds of one reference, at most

ROUTES = {
    "decim": ("fast", "generic:rate", "generic:taps", "generic:bits", "generic:shape", "generic:align"),
    "interp": ("fast", "generic:rate", "generic:taps", "generic:bits", "generic:shape", "generic:align"),
    "resample": ("fast", "forward", "generic:rate", "generic:taps", "generic:bits", "generic:shape", "generic:align"),
    "cplx": ("fast", "forward", "generic:taps", "generic:bits", "generic:stage", "generic:shape", "generic:align"),
}
# What tests/test_rate_property_cases.py requires of the derandomized draws.  The route table is one
# half fast, the other half spread evenly over the other routes: 1 / 10 or 1 / 12 each.  hypothesis
# emits a generated case about seven times over, each time with one drawn value copied over another
# (runs of one route, seen in the sequence of draws), so n draws hold about n / 7 independent
# routes: at the 1500 draws of that test a route of 1 / 12 has a standard deviation of 1.9 % and
# fast one of 3.4 %.  The bounds are three and four of those away, because the derandomized draws
# are not fixed for good: hypothesis mixes constants it finds in the project's imported modules
# into its integers, so they change with this file and with the set of modules a run imports.
MIN_SHARE, FAST_SHARE = 0.025, (0.35, 0.65)


@dataclass(frozen=True)
class Case:
    """One call.  hq: the taps as ints (complex: (hr, hi) pairs).  x_lead / y_lead: bytes past a
    512-byte boundary at which guarded_input / guarded_output place x and y."""
    family: str
    route: str
    dtype: str = "i16"  # "u8" | "i16"
    ch: int = 1
    stage: int = I32
    up: int = 1
    decim: int = 1
    phase: int = 0
    hq: tuple = (4096,)
    frac: int = 12
    acc: int = 32
    rows: int = 1
    width: int = 64
    seed: int = 0
    fill: str = "uniform"  # "uniform" | "ends" | "min" | "max"
    x_lead: int = 0
    y_lead: int = 0

    @property
    def np_dtype(self):
        return np.uint8 if self.dtype == "u8" else np.int16

    @property
    def taps(self) -> int:
        return len(self.hq)

    @property
    def out_itemsize(self) -> int:
        return 4 if self.stage == I32 else 1


# ---- samples -------------------------------------------------------------------------------------
def samples(c: Case) -> np.ndarray:
    """The (rows, width * channels) input of a case: its seed through np.random.default_rng."""
    lo, hi = (0, 255) if c.dtype == "u8" else (-32768, 32767)
    rng = np.random.default_rng(c.seed)
    shape = (c.rows, c.width * c.ch)
    if c.fill == "uniform":
        return rng.integers(lo, hi + 1, shape, dtype=c.np_dtype)
    if c.fill == "ends":
        return np.where(rng.integers(0, 2, shape) == 0, lo, hi).astype(c.np_dtype)
    return np.full(shape, lo if c.fill == "min" else hi, c.np_dtype)


# ---- references ----------------------------------------------------------------------------------
def stuff(x, U, ch):
    """x with U - 1 zero frames after every frame: (rows, width * U * ch)."""
    rows, rowlen = x.shape
    xu = np.zeros((rows, rowlen // ch * U, ch), x.dtype)
    xu[:, ::U] = x.reshape(rows, rowlen // ch, ch)
    return xu.reshape(rows, -1)


def decim_want(x, hq, D, phase, frac, acc, stage, ch):
    """(rows, out_width, ch): the oracle at full rate, sliced [:, phase::D]."""
    rows, rowlen = x.shape
    full = c_oracle().fir1d_rows(x, hq, frac, acc, stage, channels=ch).reshape(rows, rowlen // ch, ch)
    return np.ascontiguousarray(full[:, phase::D])


def interp_want(x, hq, U, frac, acc, stage, ch):
    """(rows, width * U * ch): the oracle at full rate on the stuffed signal."""
    return c_oracle().fir1d_rows(stuff(x, U, ch), hq, frac, acc, stage, channels=ch)


def resample_up(x, hq, U, frac, acc, stage, ch):
    """The full-rate result of the stuffed signal as (rows, width * U, ch): what every (D, phase) slices."""
    rows, rowlen = x.shape
    if rowlen == 0 or rows == 0:
        return np.zeros((rows, 0, ch), np.uint8 if stage == U8 else np.int32)
    return c_oracle().fir1d_rows(stuff(x, U, ch), hq, frac, acc, stage, channels=ch).reshape(rows, rowlen // ch * U, ch)


def resample_slice(up, D, phase):
    return np.ascontiguousarray(up[:, phase::D]).reshape(up.shape[0], -1)


def resample_want(x, hq, U, D, phase, frac, acc, stage, ch):
    """(rows, out_width * ch): the stuffed-signal result sliced [:, phase::D]."""
    return resample_slice(resample_up(x, hq, U, frac, acc, stage, ch), D, phase)


def want(c: Case, x: np.ndarray) -> np.ndarray:
    """What the family's entry must give for the case, as (rows, out_width * channels)."""
    if c.family == "decim":
        return decim_want(x, c.hq, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch).reshape(c.rows, -1)
    if c.family == "interp":
        return interp_want(x, c.hq, c.up, c.frac, c.acc, c.stage, c.ch)
    if c.family == "resample":
        return resample_want(x, c.hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch)
    return cplx_want(x, c.hq, c.frac, c.acc, c.stage)


def out_width(c: Case) -> int:
    """Output frames of a row, by the library's own pure host functions."""
    if c.family == "decim":
        return fir_hip.decim_out_width(c.width, c.decim, c.phase)
    if c.family == "interp":
        return fir_hip.interp_out_width(c.width, c.up)
    if c.family == "resample":
        return fir_hip.resample_out_width(c.width, c.up, c.decim, c.phase)
    return c.width


def describe_mismatch(c: Case, got: np.ndarray, ref: np.ndarray) -> str | None:
    """None when got equals ref bit for bit; else the grids' failure message with the drawn route."""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"{c.family} [{c.route}]: got {got.shape} {got.dtype}, want {ref.shape} {ref.dtype}; {c}"
    if np.array_equal(got, ref):
        return None
    bad = np.argwhere(got != ref)
    r, k = (int(v) for v in bad[0])
    m, head = k // c.ch, f"{c.family} [{c.route}]: {len(bad)} of {ref.size} values differ; the first at row {r}, "
    if c.family == "cplx":
        where = f"frame {k // 2} ({'im' if k % 2 else 're'})"
    elif c.family == "decim":
        where = f"output frame {m} (frame {m * c.decim + c.phase} of the row), channel {k % c.ch}"
    elif c.family == "interp":
        where = f"output frame {m} (input frame {m // c.up}, phase {m % c.up}), channel {k % c.ch}"
    else:
        where = (f"output frame {m} (period {m // c.up}, q {m % c.up}, frame {m * c.decim + c.phase} of the "
                 f"interpolated row), channel {k % c.ch}")
    return f"{head}{where}: got {got[r, k]}, want {ref[r, k]}; {c}"


# ---- the dispatchers, restated ---------------------------------------------------------------------
def _real_reasons(c: Case, x_addr: int, rate_ok: bool, count_ok: bool) -> list[str]:
    """Why decim_path_ok / interp_path_ok / resample_path_ok (fir1d_decim.hip:288-300,
    fir1d_interp.hip:335-348, fir1d_resample.hip:415-429; documented in fir_launch.h:84-129) refuse a
    call, in this module's order."""
    u8 = c.dtype == "u8"
    why = []
    if not rate_ok:
        why.append("generic:rate")
    if not count_ok or min(c.hq) < -32768 or max(c.hq) > 32767:
        why.append("generic:taps")
    if c.acc > 32 or c.frac > 31:
        why.append("generic:bits")
    if not (c.ch == 1 or (c.ch == 2 and not u8)) or not (c.rows == 1 or (c.width * c.ch) % 8 == 0):
        why.append("generic:shape")
    if x_addr % (8 if u8 else 16) != 0:
        why.append("generic:align")
    # the grid limits of the three predicates (width < 2^40, rows * workgroups < 2^31) lie far past
    # every drawn size
    assert c.width < 1 << 40 and c.rows * (out_width(c) // 256 + 1) < 1 << 31
    return why


def decim_route(c: Case, x_addr: int, y_addr: int = 0) -> str:
    """launch_fir1d_decim (fir1d_decim.hip:370-391): no forward; y at any element address."""
    why = _real_reasons(c, x_addr, 2 <= c.decim <= MAX_RATE, c.taps <= MAX_TAPS_REAL)
    return why[0] if why else "fast"


def interp_route(c: Case, x_addr: int, y_addr: int = 0) -> str:
    """launch_fir1d_interp (fir1d_interp.hip:414-431): no forward; y at any element address."""
    why = _real_reasons(c, x_addr, 2 <= c.up <= MAX_RATE, c.taps <= MAX_TAPS_REAL)
    return why[0] if why else "fast"


def resample_route(c: Case, x_addr: int, y_addr: int = 0) -> str:
    """launch_fir1d_resample (fir1d_resample.hip:512-538): up == 1 goes to the decimator and
    decim == 1 to the interpolator before resample_path_ok is asked."""
    if c.up == 1 or c.decim == 1:
        return "forward"
    why = _real_reasons(c, x_addr, 2 <= c.up <= MAX_RATE and 2 <= c.decim <= MAX_RATE,
                        -(-c.taps // c.up) <= MAX_PHASE_TAPS)
    return why[0] if why else "fast"


def cplx_route(c: Case, x_addr: int, y_addr: int) -> str:
    """launch_fir1d_cplx (fir1d_cplx.hip:367-389): all-real taps go to launch_fir1d_rows with two
    channels; then cplx_path_ok (fir1d_cplx.hip:280-286; fir_launch.h:136-144)."""
    parts = [int(v) for tap in c.hq for v in tap]
    if all(tap[1] == 0 for tap in c.hq):
        return "forward"
    why = []
    if c.taps > MAX_TAPS_CPLX or min(parts) < -32767 or max(parts) > 32767:
        why.append("generic:taps")
    if c.acc > 32 or c.frac > 31:
        why.append("generic:bits")
    if c.stage != I32:
        why.append("generic:stage")
    if not (c.rows == 1 or c.width % CPLX_VEC == 0):
        why.append("generic:shape")
    if x_addr % 16 != 0 or y_addr % 16 != 0:
        why.append("generic:align")
    assert c.rows * c.width < 1 << 40
    return why[0] if why else "fast"


_ROUTE_OF = {"decim": decim_route, "interp": interp_route, "resample": resample_route, "cplx": cplx_route}


def route_of(c: Case, x_addr: int, y_addr: int) -> str:
    """The route the family's dispatcher takes for the case with x and y at these addresses."""
    return _ROUTE_OF[c.family](c, x_addr, y_addr)


def forwarded_to(c: Case) -> str | None:
    """The entry a forward case is handed to: "decim", "interp" or "rows2" (the real two-channel call)."""
    if c.family == "resample" and c.up == 1:
        return "decim"
    if c.family == "resample" and c.decim == 1:
        return "interp"
    if c.family == "cplx" and all(tap[1] == 0 for tap in c.hq):
        return "rows2"
    return None


def check_sizes(c: Case) -> str | None:
    """check_fir1d (fir1d.hip:216-227) and the size rules check_fir1d_decim / _interp / _resample /
    _cplx add (fir1d_decim.hip:275-286, fir1d_interp.hip:299-309, fir1d_resample.hip:350-366,
    fir1d_cplx.hip:261-269): the refusal's text, None for a legal call."""
    i64 = (1 << 63) - 1
    parts = [int(v) for tap in c.hq for v in tap] if c.family == "cplx" else [int(v) for v in c.hq]
    if c.dtype not in ("u8", "i16") or c.stage not in (U8, I32):
        return "in_dtype / out_stage"
    if c.rows < 0 or c.width < 0 or c.ch < 1:
        return "rows, width, channels"
    if not 1 <= c.taps <= fir_hip.MAX_TAPS or min(parts) < -(1 << 31) or max(parts) >= 1 << 31:
        return "taps"
    if c.frac < 1 or c.acc < 1:
        return "frac_bits and acc_bits must be >= 1"
    if c.family == "cplx":
        return None if (c.dtype, c.ch) == ("i16", 2) and c.rows * c.width <= i64 // 8 else "rows * width * 2 * 4 bytes"
    if c.family in ("interp", "resample") and c.up < 1:
        return "up must be >= 1"
    if c.family in ("decim", "resample") and (c.decim < 1 or not 0 <= c.phase < c.decim):
        return "decim, phase"
    n_in = c.rows * c.width * c.ch
    n_out = c.rows * out_width(c) * c.ch
    return None if n_in <= i64 // 4 and n_out <= i64 // 4 and c.width * c.up <= i64 else "sizes"


# ---- geometry of the fast kernels: where passes, tiles and workgroups end, in input frames ----------
def width_edges(fam: str, dtype: str, ch: int, stage: int, U: int, D: int) -> list[int]:
    in_size, out_size = (1 if dtype == "u8" else 2), (4 if stage == I32 else 1)
    common = [8, 64, 256, 1024]  # a chunk, a wave, a block of the generic kernels
    if fam == "cplx":  # fir1d_cplx.hip header: a lane group, a wave's 256 frames, a tile, two tiles
        return [4, 256, 1024, 2048]
    if fam == "decim":  # fir1d_decim.hip header: tiles of 512 outputs, G = max(1, 16 / D) per workgroup
        G = max(1, MAX_RATE // D)
        return common + [512 * D, 2 * 512 * D, G * 512 * D]
    if fam == "interp":  # fir1d_interp.hip header, test_gpu_interp._tile
        F = 4096 // in_size
        T = F
        while T > 256 and T * U * ch * out_size > 16384:
            T //= 2
        return common + [512, T, F, 2 * F]
    P = 256  # fir1d_resample.hip header, test_gpu_resample._geom
    while P * D * in_size < 4096:
        P *= 2
    T = P
    while T > 256 and T * U * ch * out_size > 16384:
        T //= 2
    return common + [512 * D, T * D, P * D]


# ---- strategies ----------------------------------------------------------------------------------
_REASONS = {"decim": ("rate", "taps", "bits", "shape", "align"), "interp": ("rate", "taps", "bits", "shape", "align"),
            "resample": ("rate", "taps", "bits", "shape", "align"), "cplx": ("taps", "bits", "stage", "shape", "align")}
_IN_RATE = st.one_of(st.integers(2, MAX_RATE), st.integers(2, MAX_RATE), st.sampled_from([2, 3, 4, 8, 15, 16]))
_ABOVE_RATE = st.one_of(st.just(MAX_RATE + 1), st.integers(MAX_RATE + 1, TOP_RATE))
_SEED = st.integers(0, 2**32 - 1)
# tap kinds of test_gpu_property._taps, plus "ends": only the two ends of int16
_TAP_LIM = {"q412": 8192, "small": 8, "int16": 32767, "ends": 32767, "mad24": (1 << 23) - 1, "wide": (1 << 31) - 1}
_POKE_REAL = [32768, -32769, 1 << 23, -(1 << 23) - 1, (1 << 31) - 1, -(1 << 31)]
_POKE_CPLX = [-32768, 32768, -32769, 1 << 23, (1 << 31) - 1, -(1 << 31) + 1]  # -2^31 has no int32 negation (cplx_ref.want)


def _route_and_reasons(draw, fam):
    """(route, the set of reasons that hold); see the module docstring."""
    names = _REASONS[fam]
    others = [r for r in ROUTES[fam] if r != "fast"]
    table = ["fast"] * len(others) + others
    # a hashed 32-bit key, not sampled_from: the copies hypothesis makes between drawn values then
    # do not favour the table's first entries (0 still shrinks to fast)
    route = table[(draw(_SEED) * 2654435761 % 2**32 * len(table)) >> 32]
    if route == "fast":
        return route, set()
    if route == "forward":
        return route, {n for n in names if draw(st.integers(0, 4)) == 0}
    i = names.index(route.split(":")[1])
    return route, {names[i]} | {n for n in names[i + 1:] if draw(st.integers(0, 3)) == 0}


def _related(U):
    """D in the fast range with U | D, D | U or a common factor."""
    return [d for d in range(2, MAX_RATE + 1) if math.gcd(d, U) > 1] or [U]


def _rates(draw, fam, route, on):
    """(U, D, phase)."""
    U = D = 1
    if fam == "cplx":
        return 1, 1, 0
    if fam in ("decim", "interp"):
        r = draw(st.one_of(st.just(1), _ABOVE_RATE) if "rate" in on else _IN_RATE)
        U, D = (1, r) if fam == "decim" else (r, 1)
    elif route == "forward":
        which = draw(st.sampled_from(["U", "D", "UD"]))
        other = draw(_ABOVE_RATE if "rate" in on else _IN_RATE)
        U, D = {"U": (1, other), "D": (other, 1), "UD": (1, 1)}[which]
    elif "rate" in on:
        which = draw(st.sampled_from(["U", "D", "UD"]))
        U = draw(_ABOVE_RATE if "U" in which else st.integers(2, TOP_RATE))
        D = draw(_ABOVE_RATE if "D" in which else st.integers(2, TOP_RATE))
    else:
        U = draw(_IN_RATE)
        D = draw(st.one_of(_IN_RATE, st.sampled_from(_related(U))))  # coprime, common factors, U | D, D | U
    phase = draw(st.one_of(st.just(0), st.just(D - 1), st.integers(0, D - 1)))
    return U, D, phase


def _sample_type(draw, fam, on):
    """(dtype, channels, rows, ragged): ragged rows are several rows of no multiple of 8 samples."""
    if fam == "cplx":
        ragged = "shape" in on
        return "i16", 2, draw(st.integers(2, 12) if ragged else st.one_of(st.just(1), st.integers(2, 12))), ragged
    kind = draw(st.sampled_from(["ragged", "ragged", "ch3", "u8x2"])) if "shape" in on else "plain"
    if kind == "ch3":
        dtype, ch = draw(st.sampled_from(["u8", "i16"])), 3
    elif kind == "u8x2":
        dtype, ch = "u8", 2
    else:
        dtype, ch = draw(st.sampled_from([("u8", 1), ("i16", 1), ("i16", 2)]))
    rows = draw(st.integers(2, 12) if kind == "ragged" else st.one_of(st.just(1), st.integers(2, 12)))
    ragged = kind == "ragged" or (kind != "plain" and rows > 1 and draw(st.booleans()))
    return dtype, ch, rows, ragged


def _tap_count(draw, fam, U, on):
    """(L, by_value): L past the family's limit when the taps reason holds by count."""
    lmax = {"decim": MAX_TAPS_REAL, "interp": MAX_TAPS_REAL, "resample": MAX_PHASE_TAPS * U, "cplx": MAX_TAPS_CPLX}[fam]
    if "taps" in on and lmax < LONG_TAPS and draw(st.sampled_from([True, False, False])):
        return draw(st.one_of(st.just(lmax + 1), st.integers(lmax + 1, lmax + 40), st.integers(lmax + 1, LONG_TAPS))), False
    # the tap buckets of the four launchers end at these counts (decim: L + pf; interp / resample:
    # pairs per phase, so about 2 * pairs * U taps; cplx: LP)
    if fam == "decim":
        ends = [8, 16, 24, 32, 48, 64, 96]
    elif fam == "cplx":
        ends = [2, 4, 6, 8, 12, 16, 24, 32, 48]
    else:
        ends = [2 * p * U for p in (2, 3, 4, 6, 10, 14, 18, 26)]
    near = sorted({min(lmax, max(1, e + d)) for e in ends for d in (-2, -1, 0, 1)})
    L = draw(st.one_of(st.integers(1, 9), st.integers(1, min(lmax, 40)), st.integers(1, lmax), st.sampled_from(near),
                       st.sampled_from([lmax, max(1, lmax - 1)]), st.integers(1, max(1, U))))
    return L, "taps" in on


def _tap_values(draw, n, kinds, lo16):
    kind = draw(st.sampled_from(kinds))
    lim = _TAP_LIM[kind]
    lo, hi = max(-lim - 1, lo16) if lim <= 32767 else -lim, lim
    if kind == "small":
        lo = -lim
    if n <= 32:  # drawn one by one, so that a failure shrinks to readable taps
        each = st.sampled_from([lo, hi]) if kind == "ends" else st.integers(lo, hi)
        return np.asarray(draw(st.lists(each, min_size=n, max_size=n)), dtype=np.int64)
    rng = np.random.default_rng(draw(_SEED))
    if kind == "ends":
        return np.where(rng.integers(0, 2, n) == 0, lo, hi).astype(np.int64)
    return rng.integers(lo, hi + 1, n, dtype=np.int64)


def _zero_some(draw, h, period):
    """Zero taps: none, a random third, or one whole polyphase branch h[p::period]."""
    mode = draw(st.sampled_from(["none", "none", "sparse", "phase"]))
    if mode == "sparse":
        h[np.random.default_rng(draw(_SEED)).random(len(h)) < 0.3] = 0
    elif mode == "phase":
        h[draw(st.integers(0, period - 1))::period] = 0
    return h


def _taps(draw, fam, route, on, U, D):
    L, by_value = _tap_count(draw, fam, U, on)
    kinds = ["q412", "q412", "small", "int16", "ends"] + (["mad24", "wide"] if by_value else [])
    if fam != "cplx":
        h = _zero_some(draw, _tap_values(draw, L, kinds, -32768), D if fam == "decim" else U)
        if by_value:  # whatever the kind drew, one tap is outside int16
            h[draw(st.integers(0, L - 1))] = draw(st.sampled_from(_POKE_REAL))
        return tuple(int(v) for v in h)
    h = _zero_some(draw, _tap_values(draw, 2 * L, kinds, -32767), 4).reshape(L, 2)  # period 4: every other tap
    if draw(st.integers(0, 7)) == 0:
        h[:, 0] = 0  # purely imaginary taps
    if route == "forward":
        h[:, 1] = 0
    if by_value:
        h[draw(st.integers(0, L - 1)), 0 if route == "forward" else draw(st.integers(0, 1))] = draw(st.sampled_from(_POKE_CPLX))
    if route != "forward" and not h[:, 1].any():  # never all real: the call must not be forwarded
        h[L // 2, 1] = draw(st.sampled_from([1, -1, 77, 32767, -32767]))
    return tuple((int(a), int(b)) for a, b in h)


def _bits(draw, on):
    """(frac_bits, acc_bits): frac in {12} u [1, 31] u [32, 40], acc in {32} u [max(1, frac - 4), 64]."""
    low_frac = st.one_of(st.just(12), st.integers(1, 31), st.just(31))
    if "bits" not in on:
        frac = draw(low_frac)
        return frac, draw(st.one_of(st.just(32), st.integers(max(1, frac - 4), 32)))
    which = draw(st.sampled_from(["acc", "frac", "both"]))
    frac = draw(low_frac if which == "acc" else st.one_of(st.just(32), st.integers(32, 40)))
    lo = max(1, frac - 4)
    if which == "frac" and lo <= 32:
        return frac, draw(st.one_of(st.just(32), st.integers(lo, 32)))
    return frac, draw(st.one_of(st.just(33), st.integers(max(33, lo), 64)))


def _width(draw, fam, edges, rows, ch, ragged, cost_per_frame):
    """Input frames of a row: clustered on multiples of 8 samples and around the kernel's edges,
    at most MAX_WIDTH and WORK (by min(), nothing is rejected)."""
    unit = CPLX_VEC if fam == "cplx" else 8 // math.gcd(8, ch)  # frames in 8 samples (complex: a lane group)
    cap = max(1, min(MAX_WIDTH[fam], WORK // (rows * cost_per_frame)))
    w = draw(st.one_of(st.integers(1, 64), st.integers(1, cap), st.integers(1, max(1, cap // unit)).map(lambda k: k * unit),
                       st.tuples(st.sampled_from(edges), st.sampled_from([-1, 0, 1, unit, -unit])).map(sum)))
    w = max(1, min(w, cap))
    if rows > 1 and not ragged:  # rows of whole 8-sample chunks (complex: whole lane groups)
        w = max(unit, w // unit * unit)
    elif ragged and w % unit == 0:
        w += draw(st.sampled_from([1, 2, 3])) if fam == "cplx" else 1
        assert (w * (1 if fam == "cplx" else ch)) % (CPLX_VEC if fam == "cplx" else 8) != 0
    return w


def _leads(draw, fam, dtype, stage, on):
    """(x_lead, y_lead) in bytes, whole elements."""
    ysz = 4 if stage == I32 else 1
    if fam == "cplx":
        which = draw(st.sampled_from(["x", "y", "xy"])) if "align" in on else ""
        x = draw(st.sampled_from([2, 4, 6, 8, 12, 20]) if "x" in which else st.sampled_from([0, 0, 16, 32, 48, 496]))
        y = draw(st.sampled_from([1, 2, 3, 5, 6, 7, 9])) * ysz if "y" in which else draw(st.sampled_from([0, 0, 16, 32, 48]))
        assert (y % 16 != 0) == ("y" in which)
        return x, y
    if "align" in on:
        x = draw(st.sampled_from([1, 2, 3, 4, 5, 6, 7, 9, 12, 20] if dtype == "u8" else [2, 4, 6, 8, 10, 12, 14, 18, 24, 40]))
    else:
        x = draw(st.sampled_from([0, 0, 16, 32, 48, 64, 256, 496] + ([8, 24, 40] if dtype == "u8" else [])))
    return x, draw(st.integers(0, 15)) * ysz  # y at any element address


def _case(draw, fam):
    route, on = _route_and_reasons(draw, fam)
    U, D, phase = _rates(draw, fam, route, on)
    dtype, ch, rows, ragged = _sample_type(draw, fam, on)
    if fam == "cplx":
        stage = U8 if "stage" in on else I32
    else:
        stage = draw(st.sampled_from([U8, I32]))
    hq = _taps(draw, fam, route, on, U, D)
    frac, acc = _bits(draw, on)
    # multiply-adds of the reference per input frame (complex: two real filters of 4 (L / 2) + 3 taps over 2 samples)
    cost = 4 * (4 * (len(hq) // 2) + 3) if fam == "cplx" else ch * U * len(hq)
    width = _width(draw, fam, width_edges(fam, dtype, ch, stage, U, D), rows, ch, ragged, cost)
    x_lead, y_lead = _leads(draw, fam, dtype, stage, on)
    return Case(fam, route, dtype, ch, stage, U, D, phase, hq, frac, acc, rows, width, draw(_SEED),
                draw(st.sampled_from(["uniform", "uniform", "ends", "min", "max"])), x_lead, y_lead)


@st.composite
def decim_case(draw):
    return _case(draw, "decim")


@st.composite
def interp_case(draw):
    return _case(draw, "interp")


@st.composite
def resample_case(draw):
    return _case(draw, "resample")


@st.composite
def cplx_case(draw):
    return _case(draw, "cplx")


STRATEGIES = {"decim": decim_case, "interp": interp_case, "resample": resample_case, "cplx": cplx_case}


def any_case():
    """One case of any family: the host entries' test."""
    return st.one_of(decim_case(), interp_case(), resample_case(), cplx_case())


# ---- pinned examples: the thresholds a random draw reaches rarely ---------------------------------------
def _ramp(n, lo=-2000, step=37):
    return tuple(lo + step * k for k in range(n))


def _with(h, k, v):
    return h[:k] + (v,) + h[k + 1:]


def _cramp(n):
    return tuple((-1500 + 29 * k, 700 - 13 * k) for k in range(n))


def _pinned_real(fam, **rate):
    fast, mk = dict(rate), lambda route, **kw: Case(fam, route, **{**rate, **kw})
    big = {"decim": ("decim", "phase"), "interp": ("up", None), "resample": ("up", None)}[fam]
    lim = MAX_PHASE_TAPS * rate["up"] if fam == "resample" else MAX_TAPS_REAL
    at16 = {big[0]: 16, **({big[1]: 15} if big[1] else {})}
    at17 = {big[0]: 17, **({big[1]: 16} if big[1] else {})}
    h9 = _ramp(9)
    return [
        mk("fast", hq=_ramp(lim, -1000, 3), width=1032, rows=2), mk("generic:taps", hq=_ramp(lim + 1, -1000, 3), width=1032, rows=2),
        Case(fam, "fast", **{**fast, **at16}, hq=h9, width=1032, rows=3),
        Case(fam, "generic:rate", **{**fast, **at17}, hq=h9, width=1032, rows=3),
        mk("fast", hq=_with(h9, 4, 32767), width=520), mk("generic:taps", hq=_with(h9, 4, 32768), width=520),
        mk("fast", hq=_with(h9, 0, -32768), width=520, dtype="u8", stage=U8),
        mk("generic:taps", hq=_with(h9, 8, -32769), width=520, dtype="u8", stage=U8),
        mk("fast", hq=h9, acc=32, width=264, fill="ends"), mk("generic:bits", hq=h9, acc=33, width=264, fill="ends"),
        mk("fast", hq=h9, frac=31, width=264, fill="min"), mk("generic:bits", hq=h9, frac=32, width=264, fill="min"),
        mk("fast", hq=h9, rows=3, width=1032), mk("generic:shape", hq=h9, rows=3, width=1036),
        mk("fast", hq=h9, rows=3, width=516, ch=2), mk("generic:shape", hq=h9, rows=3, width=518, ch=2),
        mk("fast", hq=h9, rows=1, width=1035, y_lead=4), mk("generic:shape", hq=h9, rows=2, width=1035, y_lead=4),
        mk("fast", hq=h9, rows=2, width=264, x_lead=8, dtype="u8"), mk("generic:align", hq=h9, rows=2, width=264, x_lead=8),
    ]


PINNED = {
    "decim": _pinned_real("decim", decim=4, phase=3),
    "interp": _pinned_real("interp", up=4),
    "resample": _pinned_real("resample", up=3, decim=4, phase=3) + [
        Case("resample", "fast", up=16, decim=16, phase=15, hq=_ramp(9), width=1032, rows=2),
        Case("resample", "generic:rate", up=16, decim=17, phase=16, hq=_ramp(9), width=1032, rows=2),
        Case("resample", "forward", up=1, decim=17, phase=16, hq=_ramp(9), width=1032, rows=2),
        Case("resample", "forward", up=16, decim=1, hq=_ramp(129, -1000, 3), width=520),
        # the two calls the issue names: no grid runs either
        Case("resample", "fast", up=7, decim=12, phase=11, hq=_ramp(33), acc=19, frac=27, rows=5, width=24, y_lead=4),
        Case("resample", "generic:rate", up=17, decim=9, phase=8, hq=_ramp(9), ch=3, rows=3, width=5),
    ],
    "cplx": [
        Case("cplx", "fast", ch=2, hq=_cramp(64), width=1028, rows=2), Case("cplx", "generic:taps", ch=2, hq=_cramp(65), width=1028, rows=2),
        Case("cplx", "fast", ch=2, hq=_with(_cramp(9), 4, (-32767, 5)), width=260),
        Case("cplx", "generic:taps", ch=2, hq=_with(_cramp(9), 4, (-32768, 5)), width=260),
        Case("cplx", "fast", ch=2, hq=_with(_cramp(9), 0, (5, -32767)), width=260),
        Case("cplx", "generic:taps", ch=2, hq=_with(_cramp(9), 0, (5, -32768)), width=260),
        Case("cplx", "fast", ch=2, hq=_with(_cramp(9), 8, (32767, 32767)), width=260, fill="min"),
        Case("cplx", "generic:taps", ch=2, hq=_with(_cramp(9), 8, (32768, 1)), width=260, fill="min"),
        Case("cplx", "fast", ch=2, hq=_cramp(9), acc=32, width=260, fill="ends"),
        Case("cplx", "generic:bits", ch=2, hq=_cramp(9), acc=33, width=260, fill="ends"),
        Case("cplx", "fast", ch=2, hq=_cramp(9), frac=31, width=260), Case("cplx", "generic:bits", ch=2, hq=_cramp(9), frac=32, width=260),
        Case("cplx", "fast", ch=2, hq=_cramp(9), rows=3, width=1028), Case("cplx", "generic:shape", ch=2, hq=_cramp(9), rows=3, width=1030),
        Case("cplx", "fast", ch=2, hq=_cramp(9), rows=1, width=1031), Case("cplx", "generic:shape", ch=2, hq=_cramp(9), rows=2, width=1031),
        Case("cplx", "generic:stage", ch=2, hq=_cramp(9), rows=2, width=1028, stage=U8),
        Case("cplx", "generic:align", ch=2, hq=_cramp(9), rows=2, width=1028, y_lead=8),
        Case("cplx", "generic:align", ch=2, hq=_cramp(9), rows=2, width=1028, x_lead=2),
        Case("cplx", "forward", ch=2, hq=tuple((a, 0) for a, _ in _cramp(9)), rows=2, width=1030),
    ],
}
