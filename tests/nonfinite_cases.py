"""NaN, infinity, subnormal and signed-zero cases for the four float64 kernel families
(csrc/restore.hip, metrics.hip, ideal.hip + ideal_reg.h, ideal2d.hip) -- a test helper, not a test
module.

tests/test_gpu_nonfinite.py runs the cases on the GPU; tests/test_nonfinite_cases.py keeps this
module honest without one (every case holds what its id says, its expected output shows the
special, the two oracles agree, and the reference's recorded outputs equal the oracle's).

Inputs are built procedurally: a seeded ``default_rng`` filler plus specials at named indices, so
only expected outputs are committed (tests/golden/nonfinite.*, recorded from the reference by
tests/golden/make_nonfinite.py).  Every case has a ``plain`` twin: the same input with each
special replaced by an ordinary value.  A case whose expected output equals its twin's would pass
on a kernel that ignores the special, so the builders drop it (``shows``) and the CPU test asserts
that none is left.

The shapes are the smallest that reach each branch:

restore  n = 1 (clip only: normalize of one element is 0 whatever it holds); 255 (all scalar tail);
         256 = kRestorePerWave (one full-wave group, no tail); 257 (a full wave + a tail of 1);
         1027 (4 full waves + a tail of 3; the min/max pass gives each 256-thread workgroup 256
         pairs of samples, so workgroup 0 owns [0, 512), workgroup 1 [512, 1024), workgroup 2 the
         pair after them, and thread 0 of workgroup 0 the odd last sample).
metrics  n = 1, 7, 8 (pw_leaf's branches), 1000 (one ragged block), 2 * 8192 + 77 (two full blocks
         in one streaming workgroup + a ragged block), 9 * 8192 (three streaming workgroups of four
         waves, one block per wave: block 8 belongs to the last workgroup; no ragged block).
ideal 1-D  (1, 1030) one row, (3, 68) rows of whole 4-sample vectors, (5, 67) rows that straddle
         vectors; L <= 9 on aligned buffers is the register kernel, L = 10, 33 or x one byte off the
         generic one; L = 1030 over (2, 1500) walks two tap chunks of 1024.
ideal 2-D  (9, 20) and (70, 1028) with 3x3 / 5x5 taps: the register kernel (width a multiple of 4);
         (7, 19), and 1x7 taps, the generic one.  Finite taps only: the header leaves non-finite
         h undefined there.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from ideal2d_ref import ideal2d
from oracle import fir_oracle as fo

NAN, INF = float("nan"), float("inf")
SUB = 5e-324                       # the smallest subnormal
MIN_NORMAL = 2.2250738585072014e-308
ABOVE_255 = float(np.nextafter(255.0, np.inf))
ORDINARY = 100.25                  # what a special is replaced with in a case's plain twin


# ---- the comparison rule -------------------------------------------------------------------------
def same_f64(got, want) -> bool:
    """The NaN masks are equal and, where not NaN, the float64 bit patterns are (the sign of an
    infinity or a zero counts).  A NaN's sign and payload are not compared: x86 and the GPU make
    different default NaNs."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]))


def first_diff(got, want):
    """(flat index, got, want) of the first element the rule rejects, for an assertion message."""
    g, w = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    bad = np.flatnonzero((np.isnan(g) != np.isnan(w)) | (~np.isnan(g) & ~np.isnan(w) & (g.view(np.uint64) != w.view(np.uint64))))
    return (int(bad[0]), float(g[bad[0]]), float(w[bad[0]])) if bad.size else None


@dataclass(frozen=True)
class Case:
    id: str
    entry: str          # the fir_hip entry the case targets
    kernels: tuple      # the kernels the call must launch, in order (launch_log)
    reason: str
    args: dict = field(compare=False, hash=False, repr=False)   # the inputs
    plain: dict = field(compare=False, hash=False, repr=False)  # the same without the specials
    claims: tuple = field(default=(), compare=False, hash=False, repr=False)  # (array, index, value) the id promises


def _claims_hold(c: Case) -> bool:
    for name, idx, val in c.claims:
        got = np.asarray(c.args[name]).reshape(-1)[idx]
        if np.isnan(val):
            if not np.isnan(got):
                return False
        elif np.float64(got).view(np.uint64) != np.float64(val).view(np.uint64):
            return False
    return True


# ==== restore =====================================================================================
RESTORE_SIZES = (1, 255, 256, 257, 1024 + 3)
RESTORE_PER_WAVE = 256   # kRestorePerWave
CLIP_KINDS = (("nan", NAN), ("pinf", INF), ("ninf", -INF), ("pzero", 0.0), ("nzero", -0.0), ("psub", SUB),
              ("nsub", -SUB), ("p1e308", 1e308), ("n1e308", -1e308), ("tie254", 254.5), ("tie255", 255.5),
              ("nhalf", -0.5))
CLIP, NORMALIZE = 0, 1   # FIR_RESTORE_CLIP, FIR_RESTORE_NORMALIZE


def restore_expected(a, policy):
    with np.errstate(all="ignore"):
        return fo.to_u8_clip(a) if policy == CLIP else fo.to_u8_normalized(a)


def _filler(n, seed):
    return np.random.default_rng(seed).uniform(-300.0, 600.0, n)


def _restore_case(cid, policy, a, plain, reason, claims):
    kernels = ("restore_map_kernel",) if policy == CLIP else ("restore_minmax_kernel", "restore_params_kernel",
                                                              "restore_map_kernel")
    return Case(cid, "restore_u8", kernels, reason, {"a": a, "policy": policy}, {"a": plain, "policy": policy},
                tuple(("a", i, v) for i, v in claims))


def _restore_clip_cases():
    out = []
    for name, v in CLIP_KINDS:  # n = 1: one special each
        out.append(_restore_case(f"restore-clip-n1-{name}", CLIP, np.array([v]), np.array([ORDINARY]),
                                 f"clip of {v!r} alone (the scalar tail path)", [(0, v)]))
    for n in RESTORE_SIZES[1:]:
        # every kind at the start, in the middle and at the end: n = 255 is all scalar tail, 256 all
        # full-wave path, 257 / 1027 end in a tail of 1 / 3 (the kinds rotated so that each size's
        # last slots hold other kinds)
        a, plain, claims = _filler(n, 100 + n), _filler(n, 100 + n), []
        K = len(CLIP_KINDS)
        for base, rot in ((0, 0), (n // 2 - K // 2, 5), (n - K, n % K)):
            for i in range(K):
                v = CLIP_KINDS[(i + rot) % K][1]
                a[base + i], plain[base + i] = v, ORDINARY
                claims.append((base + i, v))
        out.append(_restore_case(f"restore-clip-n{n}-all-kinds", CLIP, a, plain,
                                 "every clip special at index 0.., mid-array and in the last slots", claims))
    return out


def _restore_normalize_cases():
    out = []

    def add(cid, a, reason, claims):
        out.append(_restore_case(f"restore-norm-{cid}", NORMALIZE, a, _filler(a.size, 7 + a.size), reason, claims))

    # (n = 1 has no normalize case: one element is its own min and max, hi <= lo or NaN, and the
    # output is 0 whatever it holds, so no input can show a special there)
    add("n2-signed-zero", np.array([-0.0, 0.0]), "[-0.0, 0.0]: hi <= lo must give zeros", [(0, -0.0), (1, 0.0)])
    # kinds placed among finite values: {name: [(offset from the position, value)]}
    placed = {"one-nan": [(0, NAN)], "pinf": [(0, INF)], "ninf": [(0, -INF)], "both-inf": [(0, INF), (1, -INF)],
              "overflow-range": [(0, 1e308), (1, -1e308)]}
    for n in RESTORE_SIZES[1:]:
        if n == 1027:  # the special in another min/max workgroup than the extremes, both ways round
            spots = {"wg1-extremes-wg0": (800, (3, 5)), "wg0-extremes-wg1": (7, (800, 900)), "tail": (n - 2, (3, 800))}
        else:
            spots = {"first": (0, (n // 3, n // 3 + 1)), "mid": (n // 2, (2, 3)), "last": (n - 2, (2, n // 2))}
            if n == 255:
                del spots["mid"]   # all of it is the scalar tail
            if n == 256:
                del spots["last"]  # all of it is the full-wave path
        for kind, specials in placed.items():
            for where, (pos, ext) in spots.items():
                a = _filler(n, 1000 + n)
                a[ext[0]], a[ext[1]] = -1000.0, 2000.0  # the finite extremes
                claims = []
                for off, v in specials:
                    a[pos + off] = v
                    claims.append((pos + off, v))
                add(f"n{n}-{kind}-{where}", a, f"{kind} at {pos} ({where}) among finite values", claims)
        add(f"n{n}-all-nan", np.full(n, NAN), "all NaN", [(0, NAN), (n - 1, NAN)])
        add(f"n{n}-constant", np.full(n, 42.25), "a constant array: hi <= lo, zeros", [(0, 42.25)])
        add(f"n{n}-signed-zero", np.resize(np.array([-0.0, 0.0]), n), "-0.0 / 0.0 alternating: hi <= lo, zeros",
            [(0, -0.0), (1, 0.0)])
        add(f"n{n}-subnormal-range", np.resize(np.array([SUB, 0.0, 2 * SUB]), n),
            "range 1e-323: the scale 255 / 1e-323 is inf, 0 * inf = NaN -> 0, the rest 255",
            [(0, SUB), (1, 0.0), (2, 2 * SUB)])
        big = np.resize(np.array([1e308, -1e308, 0.0, SUB]), n)
        add(f"n{n}-overflow-subnormal", big, "hi - lo overflows to inf: the scale is 0, all zeros",
            [(0, 1e308), (1, -1e308)])
    return out


# ==== metrics =====================================================================================
METRIC_SIZES = (1, 7, 8, 1000, 2 * 8192 + 77, 9 * 8192)
PW_BLOCK = 8192
# form -> (fixed dtype, fixed one byte off a 16-byte boundary)
METRIC_FORMS = {"u8": (np.uint8, False), "u8off1": (np.uint8, True), "i16": (np.int16, False),
                "f16": (np.float16, False), "f32": (np.float32, False), "f64": (np.float64, False)}


def metrics_kernels(form: str, n: int) -> tuple:
    """launch_metrics_t restated: the kernels of one call."""
    nbf, ragged = n // PW_BLOCK, n % PW_BLOCK != 0
    if form == "u8" and nbf > 0:
        return ("metrics_prep", "metrics_leaf_kernel")
    blocks = () if nbf == 0 else (("metrics_blocks",) if form == "u8off1" else ("metrics_blocks_any",))
    return blocks + (("metrics_ragged",) if ragged else ()) + ("metrics_final",)


def metrics_expected(ideal, fixed) -> dict:
    with np.errstate(all="ignore"):
        return fo.compute_metrics(ideal, fixed)


def _metric_kinds(n: int, floating: bool) -> list:
    """[(kind, {ideal index: value}, {fixed index: value}, reason)] that fit n samples."""
    kinds = []

    def ideal(kind, spec, reason):
        if all(0 <= i < n for i in spec) and len(spec) == len(set(spec)):
            kinds.append((kind, dict(spec), {}, reason))

    ideal("nan-at-0", {0: NAN}, "a NaN in the ideal at index 0: max and the three means are NaN")
    if n >= 1000:
        ideal("nan-at-127", {127: NAN}, "a NaN in the last sample of leaf 0")
        ideal("nan-at-128", {128: NAN}, "a NaN in the first sample of leaf 1")
    if n > PW_BLOCK:
        ideal("nan-at-8191", {8191: NAN}, "a NaN in the last sample of block 0")
        ideal("nan-at-8192", {8192: NAN}, "a NaN in the first sample of block 1")
    if n == 9 * PW_BLOCK:
        ideal("nan-last-workgroup", {8 * PW_BLOCK + 4000: NAN}, "a NaN in block 8, owned by the last streaming workgroup")
    if n % PW_BLOCK and n > 1:
        ideal("nan-ragged-tail", {n - 1: NAN}, "a NaN only in the ragged last block, which the chain adds last")
    ideal("pinf-alone", {n // 2: INF}, "+inf alone: max, mae, rmse inf, mean_err -inf")
    if n > PW_BLOCK:
        ideal("pinf-ninf-blocks", {5: INF, PW_BLOCK + 5: -INF},
              "+inf and -inf in different blocks: sum d is NaN, sum|d| inf, so max stays inf")
    elif n >= 7:
        ideal("pinf-ninf", {0: INF, n - 1: -INF}, "+inf and -inf: sum d is NaN, sum|d| inf, so max stays inf")
    ideal("d2-overflow", {n // 3: 1e200}, "d^2 overflows while |d| is finite: rmse inf, mae finite")
    ideal("nzero-nsub", {0: -0.0, n - 1: -SUB} if n > 1 else {0: -SUB},
          "-0.0 and -5e-324 in the ideal: only the second is < 0")
    ideal("above-255", {n // 2: ABOVE_255}, "nextafter(255, inf) counts as > 255")
    if floating:
        seam = [i for i in (127, 128, 8191, 8192) if i < n] or [0]
        for name, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF), ("nzero", -0.0)):
            kinds.append((f"fixed-{name}", {}, {i: v for i in seam}, f"{v!r} in the fixed array at {seam}"))
    return kinds


@functools.lru_cache(maxsize=None)
def _metric_filler(n: int):
    rng = np.random.default_rng(4000 + n)
    return rng.uniform(1.0, 254.0, n), rng.integers(0, 256, n)


def _metrics_cases():
    out = []
    for form, (dtype, off1) in METRIC_FORMS.items():
        floating = np.issubdtype(dtype, np.floating)
        for n in METRIC_SIZES:
            for kind, ispec, fspec, reason in _metric_kinds(n, floating):
                yi0, yf0 = _metric_filler(n)
                yi, yf = yi0.copy(), yf0.astype(dtype)
                pi, pf = yi0.copy(), yf0.astype(dtype)
                claims = []
                for i, v in ispec.items():
                    yi[i], pi[i] = v, ORDINARY
                    claims.append(("ideal", i, v))
                for i, v in fspec.items():
                    yf[i], pf[i] = v, 100
                    claims.append(("fixed", i, v))
                out.append(Case(f"metrics-{form}-n{n}-{kind}", "compare_metrics", metrics_kernels(form, n), reason,
                                {"ideal": yi, "fixed": yf, "form": form, "off1": off1},
                                {"ideal": pi, "fixed": pf, "form": form, "off1": off1}, tuple(claims)))
    return out


# ==== ideal, 1-D ==================================================================================
IDEAL_SHAPES = ((1, 1030), (3, 68), (5, 67))
IDEAL_REG_L = (1, 3, 5, 9)
IDEAL_GENERIC_L = (10, 33)
IDEAL_LONG = ((2, 1500), 1030)   # two tap chunks of kIdealChunk = 1024
FINITE_SETS = {"overflow-cancel": [1.7e308, -1.7e308, 1.0], "overflow-sum": [1e308, 1e308],
               "subnormal": [SUB, 2.5e-308, -SUB], "min-normal-nzero": [MIN_NORMAL, -0.0, 1.0]}
NONFINITE_SETS = {"pinf-first": ("first", INF), "pinf-centre": ("centre", INF), "pinf-last": ("last", INF),
                  "ninf-centre": ("centre", -INF), "nan-centre": ("centre", NAN)}


@functools.lru_cache(maxsize=None)
def ideal_x(shape) -> np.ndarray:
    """uint8 rows: random, with 0, 1 and 255 at fixed positions including both ends of every row."""
    rows, width = shape
    x = np.random.default_rng(rows * 10007 + width).integers(0, 256, shape, dtype=np.uint8)
    for r in range(rows):
        x[r, 0], x[r, -1] = (0, 1, 255)[r % 3], (255, 0, 1)[r % 3]
        x[r, 10:13] = (0, 1, 255)
        x[r, width // 2:width // 2 + 3] = (255, 0, 1)
        # one sample alone in a run of zeros: the outputs around it are a single product h[k] * x, so
        # a subnormal tap shows even among ordinary taps (elsewhere their products absorb it)
        lo, hi, spike = (100, 201, 150) if width >= 1000 else (20, 41, 30)
        x[r, lo:hi] = 0
        x[r, spike] = (255, 1)[r % 2]
    x.setflags(write=False)
    return x


def _place(L: int, extreme: list, where: str, seed: int):
    """L taps: ``extreme`` (cut to L) first / centred / last among ordinary taps; and its positions."""
    ext = list(extreme)[:L]
    h = np.random.default_rng(seed).uniform(-8.0, 8.0, L)
    at = {"first": 0, "centre": (L - len(ext)) // 2, "last": L - len(ext)}[where]
    h[at:at + len(ext)] = ext
    return h, list(range(at, at + len(ext)))


def ideal_kernel(L: int, off1: bool) -> str:
    return "fir1d_ideal_reg_kernel" if L <= 9 and not off1 else "fir1d_ideal_kernel"


def ideal_expected(x, h):
    with np.errstate(all="ignore"):
        return fo.fir1d_ideal_rows(x, h)


def _ideal_cases():
    out, seen = [], set()
    geometry = [(s, L) for s in IDEAL_SHAPES for L in IDEAL_REG_L + IDEAL_GENERIC_L] + [IDEAL_LONG]
    for shape, L in geometry:
        sets = [(name, ext, where, True) for name, ext in FINITE_SETS.items() for where in ("first", "centre", "last")]
        sets += [(name, [v], where, False) for name, (where, v) in NONFINITE_SETS.items()]
        for name, ext, where, finite in sets:
            h, at = _place(L, ext, where, L * 31 + len(name))
            key = (shape, L, name, tuple(at))
            if key in seen:   # (the set fills all L taps: first = centre = last)
                continue
            seen.add(key)
            plain = h.copy()
            plain[at] = 0.0
            tag = f"{name}-{where}" if finite else name
            out.append(Case(f"ideal1d-{shape[0]}x{shape[1]}-L{L}-{tag}", "fir1d_ideal_rows", (ideal_kernel(L, False),),
                            f"taps {ext[:L]!r} at {where} of {L}" + ("" if finite else " (C ABI / fir_hip entries only)"),
                            {"shape": shape, "h": h, "finite": finite}, {"shape": shape, "h": plain, "finite": finite},
                            tuple(("h", i, h[i]) for i in at)))
    return out


# the one fir1d_ideal_images_multi call: two images, the four finite sets as 3-tap filters
IMAGES_MULTI = {"shapes": ((3, 68), (5, 67)),
                "hs": [FINITE_SETS["overflow-cancel"], FINITE_SETS["overflow-sum"] + [0.5], FINITE_SETS["subnormal"],
                       FINITE_SETS["min-normal-nzero"]]}


# ==== ideal, 2-D ==================================================================================
IDEAL2D_GEOMETRY = (((9, 20), 3, 3, "fir2d_ideal_reg_kernel"), ((9, 20), 5, 5, "fir2d_ideal_reg_kernel"),
                    ((70, 1028), 3, 3, "fir2d_ideal_reg_kernel"), ((70, 1028), 5, 5, "fir2d_ideal_reg_kernel"),
                    ((7, 19), 3, 3, "fir2d_ideal_generic_kernel"), ((7, 19), 5, 5, "fir2d_ideal_generic_kernel"),
                    ((9, 20), 1, 7, "fir2d_ideal_generic_kernel"), ((7, 19), 1, 7, "fir2d_ideal_generic_kernel"))
FRAMES = 2


@functools.lru_cache(maxsize=None)
def ideal2d_x(shape) -> np.ndarray:
    """A batch of FRAMES uint8 frames: random, with 0, 1, 255 in the corners and the middle."""
    H, W = shape
    x = np.random.default_rng(H * 7919 + W).integers(0, 256, (FRAMES, H, W), dtype=np.uint8)
    for f in range(FRAMES):
        x[f, 0, 0], x[f, 0, -1], x[f, -1, 0], x[f, -1, -1] = 0, 255, 1, (0, 255)[f]
        x[f, H // 2, W // 2 - 1:W // 2 + 2] = (255, 0, 1)
        # one sample alone in a square of zeros (see ideal_x); a small frame gives it all its rows
        if H >= 64:
            x[f, 20:33, 100:113] = 0
            x[f, 26, 106] = (255, 1)[f]
        else:
            x[f, :, 3:16] = 0
            x[f, H // 2, 9] = (255, 1)[f]
    x.setflags(write=False)
    return x


def ideal2d_expected(x, h2):
    with np.errstate(all="ignore"):
        return np.stack([ideal2d(f, h2) for f in x])


def _ideal2d_cases():
    out = []
    for shape, R, C, kernel in IDEAL2D_GEOMETRY:
        for name, ext in FINITE_SETS.items():
            for where in ("first", "centre", "last"):
                h, at = _place(R * C, ext, where, R * 100 + C + len(name))
                plain = h.copy()
                plain[at] = 0.0
                out.append(Case(f"ideal2d-{shape[0]}x{shape[1]}-{R}x{C}-{name}-{where}", "fir2d_ideal", (kernel,),
                                f"taps {ext!r} at {where} of the {R}x{C} kernel (row-major)",
                                {"shape": shape, "h2": h.reshape(R, C)}, {"shape": shape, "h2": plain.reshape(R, C)},
                                tuple(("h2", i, h[i]) for i in at)))
    return out


# ==== all cases ===================================================================================
_EXPECTED: dict = {}


def expected(c: Case, args=None):
    """The oracle's output of a case (of its plain twin with args=c.plain); computed once per case
    and shared, so treat it as read-only."""
    if args is None:
        if c.id not in _EXPECTED:
            _EXPECTED[c.id] = expected(c, c.args)
        return _EXPECTED[c.id]
    a = args
    if c.entry == "restore_u8":
        return restore_expected(a["a"], a["policy"])
    if c.entry == "compare_metrics":
        return metrics_expected(a["ideal"], a["fixed"])
    if c.entry == "fir1d_ideal_rows":
        return ideal_expected(ideal_x(a["shape"]), a["h"])
    return ideal2d_expected(ideal2d_x(a["shape"]), a["h2"])


def same_output(c: Case, got, want) -> bool:
    if c.entry == "restore_u8":
        return bool(np.array_equal(got, want))
    if c.entry == "compare_metrics":
        from conftest import same_metrics

        return not same_metrics(got, want)
    return same_f64(got, want)


def shows(c: Case) -> bool:
    """The expected output differs from the plain twin's: a kernel that ignored the special fails."""
    return not same_output(c, expected(c, c.plain), expected(c))


@functools.lru_cache(maxsize=None)
def built() -> tuple:
    """(every case that shows its special, the ids of the ones dropped because they do not)."""
    every = _restore_clip_cases() + _restore_normalize_cases() + _metrics_cases() + _ideal_cases() + _ideal2d_cases()
    keep = [c for c in every if shows(c)]
    return tuple(keep), tuple(c.id for c in every if not shows(c))


def cases(entry: str | None = None) -> list:
    return [c for c in built()[0] if entry is None or c.entry == entry]
