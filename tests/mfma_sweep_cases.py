"""Cases, launch geometry and pooled references for the steady state of the three persistent 1-D
matrix-core kernels of csrc/fir1d_mfma.hip -- a test helper, not a test module.

tests/test_gpu_mfma_sweeps.py runs the cases on the GPU; tests/test_mfma_sweep_cases.py keeps this
module honest without one.

The kernels are grid-stride loops over WORK UNITS with a software pipeline between one iteration of
a wave and the next (a window prefetched one step ahead, a ring of LDS-DMA buffers kDepth deep,
counted waits, a row / column cursor stepped with a carry).  A wave reaches its second iteration
only when a launch has more units than one sweep of the capped grid:

    kernel  unit              units of rows x rowlen                            waves of a launch
    step    step of 2 tiles   nsteps = rows * ceil(ceil(rowlen / 1024) / 2)     4 min(ceil(nsteps / 4), kMf2Blocks)
    run     run of tps tiles  nruns = ceil(ntiles / tps)                        4 min(ceil(nruns / 4), 256 w)
    long    tile              ntiles = rows * ceil(rowlen / 1024)               4 min(ceil(ntiles / 4), kMlBlocks)

(tps and w: ``run_form`` and ``mr_waves_of``, restated from launch_mfma_run and mr_waves_of; one row
is rows = 1 with rowlen = the whole signal).  Unit u is wave u % waves' iteration u // waves.

REQUIRED iterations of every wave, from the loops' structure:
    step  4   the entry edge, two loop-backs, the exit edge with its self-reload
    run   6   the ring of up to max kDepth + 1 = 4 buffers wraps, plus a steady iteration each side
    long  3   first, middle, last
Every shape has REQUIRED + 1/2 sweeps of units, so the waves of the last, half-full sweep do one
iteration more than the others and end at another ring position.

Shapes.  Iterations depend on units, not samples, so many short rows reach the steady state with
a few megabytes:
    narrow  (R, 72)    one partial tile per row, the filter's window mostly outside the row; runs of
                       2 and 4 tiles span several rows, and R is chosen so that the last run is partial
    ragged  (R, 1032)  a full tile and one of 8 samples
    full    (R, 4096)  interior tiles with neighbours on both sides (4 tiles a row: the tile count is
                       a multiple of every tps, so the partial last run is narrow's business)
    flat    (1, N)     one long row, N = REQUIRED + 1/2 sweeps + 8 samples; its reference is the
                       direct oracle (N * L multiply-adds), so only two cases use it

Pooled images.  x = pool[idx]: K = 127 distinct rows over the type's whole range (row 0 at the
type's minimum, row 1 at its maximum; u8: row 2 all 0 as well, and row 3 all 128, the zero of the
signed-byte planes), idx drawn uniformly.  Rows are filtered independently with zero padding, so
the exact reference of row r is the oracle's row idx[r] of oracle(pool): the oracle runs on K rows
whatever R is, and the expansion and the comparison stay on the device.

``stale_share``: a kernel that computed an iteration on a window left over from an earlier one
(the wrong ring buffer, a prefetch that never advanced) still passes wherever the two windows
are equal, i.e. where the tiles have the same pool row and the same column.  The share of such
tile pairs among units u and u + d * waves, d = 1..4 (the ring is at most 4 deep), must stay under
STALE_CAP; by construction it is about 1 / K = 0.8 %.  Pool rows of equal content (u8 rows 0 and 2)
count as the same row (``canonical``).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fir_hip
from oracle import c_oracle
from test_gpu_long_taps import RUN_KERNEL, _high_plane_form, _mixed_plane_filters, _run_launch  # noqa: F401

U8, I32 = fir_hip.OUT_U8_SAT, fir_hip.OUT_I32

# The constants the restatement rests on, as the sources state them
# (tests/test_mfma_sweep_cases.py reads them back from the files named here).
LIMITS = {
    "kMfTile": ("fir1d_mfma.hip", 1024),
    "kMf2Tps": ("fir1d_mfma.hip", 2), "kMf2Blocks": ("fir1d_mfma.hip", 2048),
    "kMlBlocks": ("fir1d_mfma.hip", 2048), "kMlChunk": ("fir1d_mfma.hip", 16),
    "kMrTps": ("fir1d_mfma.hip", 2), "kMrMTps": ("fir1d_mfma.hip", 4),
    "kMrC": ("fir1d_mfma.hip", 16), "kMrU8One": ("fir1d_mfma.hip", 32), "kMrMNsMin": ("fir1d_mfma.hip", 6),
    "kMrWaves": ("fir1d_mfma.hip", 2), "kMrMWaves": ("fir1d_mfma.hip", 2),
    "kMrW4Ns": ("fir1d_mfma.hip", 8), "kMrW3Ns": ("fir1d_mfma.hip", 12), "kMrW2Ns": ("fir1d_mfma.hip", 24),
    "kMrT1Ns": ("fir1d_mfma.hip", 32),
    "kMrDepth": ("fir1d_mfma.hip", 2), "kMrDepth1": ("fir1d_mfma.hip", 3), "kMrMDepth": ("fir1d_mfma.hip", 1),
    "kMfmaMinTaps": ("fir1d.hip", 10), "kMfmaMinTapsI32": ("fir1d.hip", 40),
}
# Literals of the sources that have no name there: (file, the text that must occur in it)
LITERALS = {
    "run grid cap": ("fir1d_mfma.hip", "const int64_t cap = (int64_t)256 * mr_waves_of(STAGE, tps, multi, ns);"),
    "int32 out: 3 waves up to 11 k-steps": ("fir1d_mfma.hip", "ns <= (stage == FIR_OUT_U8_SAT ? kMrW3Ns : 11) ? 3"),
    "one-tile runs, int32 out: depth 3": ("fir1d_mfma.hip", "TPS == 1 ? (OLDS ? 3 : kMrDepth1) : TPS == 4 ? kMrMDepth : kMrDepth"),
    "4 waves per workgroup": ("fir_common.h", "constexpr int kBlock = 256;"),
    "FAST needs frac <= 22": ("fir1d_mfma.hip", "const bool fast = frac <= 22 && habs * xmax + ((int64_t)1 << (frac - 1)) < "
                                                  "((int64_t)1 << (acc_bits - 1));"),
}
TILE = 1024          # kMfTile
WG_WAVES = 4         # kMfWaves = kBlock / kWave
STEP_TPS = 2         # kMf2Tps
STEP_BLOCKS = 2048   # kMf2Blocks
LONG_BLOCKS = 2048   # kMlBlocks
LONG_CHUNK = 16      # kMlChunk
RUN_BLOCKS_PER_WAVE = 256
MAX_DEPTH = 3        # max(kMrDepth, kMrDepth1, kMrMDepth, the int32 stage's 3)

REQUIRED = {"step": 4, "run": MAX_DEPTH + 1 + 2, "long": 3}
STALE_CAP = 0.03
K_POOL = 127
ROWLEN = {"narrow": 72, "ragged": 1032, "full": 4096}
# frac_bits, acc_bits, the taps' amplitude: the three forms the launchers distinguish, with the
# parameters of test_gpu_long_taps.test_u8_long_filter_run_kernel_vs_oracle
MODES = {"fast": (12, 32, 400), "acc24": (16, 24, 3000), "wrap32": (12, 32, 32639)}
IN_NAME = {"u8": "unsigned char", "i16": "short"}
NP_DTYPE = {"u8": np.uint8, "i16": np.int16}


# ---- the launchers, restated -------------------------------------------------------------------------
def k_steps(L: int, halo_round: int = 8) -> int:
    """KS of launch_mfma_t: K = 32 + L/2 + P over 32, P the left halo rounded up to 8 (the run
    kernel: 16)."""
    c = L // 2
    P = (L - 1 - c + halo_round - 1) & ~(halo_round - 1)
    return (32 + c + P + 31) // 32


def kernel_of(dtype: str, L: int) -> str:
    """launch_mfma_t: up to 3 k-steps the step kernel; past it u8 the run kernel, int16 the chunked one."""
    return "step" if k_steps(L) <= 3 else "run" if dtype == "u8" else "long"


def mfma_min_taps(dtype: str, stage: int) -> int:
    """fir1d.hip launch_fir1d_rows: the shortest filter the matrix cores take."""
    return LIMITS["kMfmaMinTapsI32"][1] if dtype == "i16" and stage == I32 else LIMITS["kMfmaMinTaps"][1]


def _run_ns(KS: int, multi_max: int, one_max: int) -> int:
    """mfma_run_ns."""
    if KS <= 12:
        return max(4, KS)
    if KS <= one_max:
        return (KS + 1) & ~1
    best, pad = multi_max, -(-KS // multi_max) * multi_max
    for ns in range(multi_max - 2, (LIMITS["kMrMNsMin"][1] if multi_max <= 8 else 8) - 1, -2):
        p = -(-KS // ns) * ns
        if p < pad:
            best, pad = ns, p
    return best


def run_form(L: int, stage: int) -> tuple:
    """(NS, several chunks, tiles per run) of launch_mfma_run<STAGE> for L taps: RUN_KERNEL's entries."""
    KS = k_steps(L, 16)
    mtps = LIMITS["kMrMTps"][1] if stage == U8 else LIMITS["kMrTps"][1]
    one_max = LIMITS["kMrU8One"][1] if stage == U8 else LIMITS["kMrC"][1]
    ns = _run_ns(KS, 8 if mtps == 4 else LIMITS["kMrC"][1], one_max)
    multi = -(-KS // ns) * ns > ns
    tps = 1 if not multi and ns <= LIMITS["kMrT1Ns"][1] else mtps if multi else LIMITS["kMrTps"][1]
    return ns, multi, tps


def mr_waves_of(stage: int, tps: int, multi: bool, ns: int) -> int:
    """Waves per SIMD of the run kernel (its launch bounds, and its grid cap over 256)."""
    if multi:
        return LIMITS["kMrMWaves"][1]
    if tps != 1:
        return LIMITS["kMrWaves"][1]
    if ns <= LIMITS["kMrW4Ns"][1] and stage == U8:
        return 4
    if ns <= (LIMITS["kMrW3Ns"][1] if stage == U8 else 11):
        return 3
    return 2 if ns <= LIMITS["kMrW2Ns"][1] else 1


def run_depth(stage: int, tps: int) -> int:
    """kDepth of the run kernel: iterations of windows in flight; its ring has one buffer more."""
    if tps == 1:
        return 3 if stage == I32 else LIMITS["kMrDepth1"][1]
    return LIMITS["kMrMDepth"][1] if tps == 4 else LIMITS["kMrDepth"][1]


def is_fast(dtype: str, hq, frac: int, acc: int) -> bool:
    """launch_mfma_t's FAST: no sum can wrap acc_bits, nor overflow int32 with the rounding half."""
    habs = sum(abs(int(v)) for v in hq)
    return frac <= 22 and habs * (255 if dtype == "u8" else 32768) + (1 << (frac - 1)) < 1 << (acc - 1)


def form_of(dtype: str, hq, frac: int, acc: int) -> str:
    """"fast" | "acc32" | "accN": the launch note's mode= of the run kernel; (ACC32, FAST) of the others."""
    return "fast" if is_fast(dtype, hq, frac, acc) else f"acc{acc}"


# ---- cases ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kernel: str          # "step" | "run" | "long"
    dtype: str           # "u8" | "i16"
    stage: int
    L: int
    shape: str           # "narrow" | "ragged" | "full" | "flat"
    mode: str            # a key of MODES
    filt: str = "random"  # or a name of test_gpu_long_taps._mixed_plane_filters (the high-plane forms)
    hn: int = -1         # the run kernel's HN the filter takes

    @property
    def id(self) -> str:
        f = "" if self.filt == "random" else f"-{self.filt}"
        return f"{self.dtype}-{'u8' if self.stage == U8 else 'i32'}-L{self.L}-{self.shape}-{self.mode}{f}"

    @property
    def tps(self) -> int:
        return STEP_TPS if self.kernel == "step" else run_form(self.L, self.stage)[2] if self.kernel == "run" else 1

    @property
    def cap_waves(self) -> int:
        """Waves of a capped launch: one sweep."""
        if self.kernel == "step":
            return WG_WAVES * STEP_BLOCKS
        if self.kernel == "long":
            return WG_WAVES * LONG_BLOCKS
        ns, multi, tps = run_form(self.L, self.stage)
        return WG_WAVES * RUN_BLOCKS_PER_WAVE * mr_waves_of(self.stage, tps, multi, ns)


@dataclass(frozen=True)
class Geometry:
    rows: int
    rowlen: int
    tiles_per_row: int
    ntiles: int
    units: int
    waves: int


def units_of(kernel: str, tps: int, rows: int, rowlen: int) -> int:
    tpr = -(-rowlen // TILE)
    if kernel == "step":
        return rows * -(-tpr // STEP_TPS)
    return -(-rows * tpr // tps)


def geometry(c: Case) -> Geometry:
    """The case's image and the launch the restated launcher gives it: REQUIRED + 1/2 sweeps of units."""
    target = (2 * REQUIRED[c.kernel] + 1) * c.cap_waves // 2
    tps = c.tps
    if c.shape == "flat":  # whole tiles of one row, and one of 8 samples
        rows, rowlen = 1, target * tps * TILE + 8
    elif c.kernel == "step":  # a step never leaves its row: ceil(tiles per row / 2) steps a row
        rowlen = ROWLEN[c.shape]
        rows = target // -(-(-(-rowlen // TILE)) // STEP_TPS)
    else:
        rowlen = ROWLEN[c.shape]
        tpr = -(-rowlen // TILE)
        ntiles = target * tps
        if tps > 1 and tpr < tps:
            ntiles -= 1  # the last run is partial
        rows = -(-ntiles // tpr)
    tpr = -(-rowlen // TILE)
    units = units_of(c.kernel, tps, rows, rowlen)
    cap = c.cap_waves // WG_WAVES
    return Geometry(rows, rowlen, tpr, rows * tpr, units, WG_WAVES * min(-(-units // WG_WAVES), cap))


def iterations(launch, units: int) -> tuple:
    """(fewest, most) iterations of a wave of a recorded launch (a fir_hip.Launch) over `units`
    work units: unit u is wave u % waves' iteration u // waves."""
    waves = launch.grid[0] * WG_WAVES
    return units // waves, -(-units // waves)


def unit_of(c: Case, g: Geometry, row: int, col: int) -> tuple:
    """(tile, unit) of output sample (row, col)."""
    tile = row * g.tiles_per_row + col // TILE
    if c.kernel == "step":
        return tile, row * -(-g.tiles_per_row // STEP_TPS) + col // TILE // STEP_TPS
    return tile, tile // c.tps


def first_sweep_outputs(c: Case, g: Geometry, waves: int) -> int:
    """The outputs of units 0 .. waves - 1, every wave's first iteration: a prefix of the image."""
    if c.kernel == "step":
        upr, per = -(-g.tiles_per_row // STEP_TPS), STEP_TPS * TILE
    else:
        upr, per = g.tiles_per_row, TILE
        waves *= c.tps
    return min(g.rows * g.rowlen, waves // upr * g.rowlen + min(waves % upr * per, g.rowlen))


@functools.lru_cache(maxsize=None)
def taps(c: Case) -> tuple:
    """The case's taps; (stage and shape share them: the seed is the length, mode and filter)."""
    rng = np.random.default_rng([c.L, sorted(MODES).index(c.mode)])
    if c.filt != "random":
        return tuple(int(v) for v in _mixed_plane_filters(c.L, np.random.default_rng(1000 + c.L))[c.filt])
    amp = MODES[c.mode][2]
    return tuple(int(v) for v in rng.integers(-amp, amp + 1, c.L))


def expected_launch(c: Case) -> tuple:
    """(kernel name, its leading template arguments, the launch note's mode or None)."""
    frac, acc, _ = MODES[c.mode]
    form = form_of(c.dtype, taps(c), frac, acc)
    acc32, fast = ("true" if form in ("fast", "acc32") else "false"), ("true" if form == "fast" else "false")
    if c.kernel == "step":
        return "fir1d_mfma_step_kernel", (IN_NAME[c.dtype], str(c.stage), str(k_steps(c.L)), acc32, fast), None
    if c.kernel == "long":
        return "fir1d_mfma_long_kernel", (IN_NAME[c.dtype], str(c.stage), acc32, fast), None
    ns, multi, tps = run_form(c.L, c.stage)
    return "fir1d_mfma_run_kernel", (str(c.stage), str(ns), "true" if multi else "false", str(tps), str(c.hn)), form


# ---- pooled images -------------------------------------------------------------------------------------
def pooled(rng, dtype, rows: int, rowlen: int, K: int = K_POOL) -> tuple:
    """(pool, idx): the image is pool[idx]; see the module docstring."""
    info = np.iinfo(dtype)
    pool = rng.integers(info.min, info.max + 1, (K, rowlen), dtype=dtype)
    pool[0], pool[1] = info.min, info.max
    if np.dtype(dtype) == np.uint8:
        pool[2], pool[3] = 0, 128
    return pool, rng.integers(0, K, rows)


def canonical(pool: np.ndarray) -> np.ndarray:
    """Pool row -> the first pool row of the same content."""
    first = {}
    return np.asarray([first.setdefault(row.tobytes(), k) for k, row in enumerate(pool)])


def stale_share(idx, tiles_per_row: int, tps: int, waves: int, rowwise: bool = False) -> float:
    """The share of tile pairs (tile q of unit u, tile q of unit u + d * waves), d = 1..4, that have
    the same pool row and the same column: where a kernel that computed on an earlier iteration's
    window would go unnoticed.  idx: each row's (canonical) pool row.  rowwise: units are the step
    kernel's, ceil(tiles_per_row / tps) to a row; else runs of tps tiles of the whole image."""
    idx = np.asarray(idx)
    rows = len(idx)
    if rowwise:
        upr = -(-tiles_per_row // tps)
        u = np.arange(rows * upr)[:, None]
        row, col = u // upr, u % upr * tps + np.arange(tps)[None, :]
        ok = col < tiles_per_row
    else:
        ntiles = rows * tiles_per_row
        t = np.arange(-(-ntiles // tps))[:, None] * tps + np.arange(tps)[None, :]
        ok = t < ntiles
        t = np.minimum(t, ntiles - 1)
        row, col = t // tiles_per_row, t % tiles_per_row
    src = idx[row]
    same = pairs = 0
    for d in range(1, 5):
        s = d * waves
        if s >= len(src):
            break
        both = ok[:-s] & ok[s:]
        pairs += int(both.sum())
        same += int((both & (src[:-s] == src[s:]) & (col[:-s] == col[s:])).sum())
    return same / pairs if pairs else 0.0


@functools.lru_cache(maxsize=None)
def pool_of(dtype: str, shape: str) -> np.ndarray:
    """The one pool of a sample type and row length, shared by every case of that shape."""
    pool, _ = pooled(np.random.default_rng([NP_DTYPE[dtype]().itemsize, ROWLEN[shape]]), NP_DTYPE[dtype], 0, ROWLEN[shape])
    pool.setflags(write=False)
    return pool


def image_index(c: Case, rows: int) -> np.ndarray:
    """idx of the case's image pool_of(c.dtype, c.shape)[idx]."""
    return np.random.default_rng([c.L, c.stage, rows]).integers(0, K_POOL, rows)


def flat_signal(c: Case, n: int) -> np.ndarray:
    info = np.iinfo(NP_DTYPE[c.dtype])
    return np.random.default_rng(c.L).integers(info.min, info.max + 1, (1, n), dtype=NP_DTYPE[c.dtype])


def reference(c: Case, x: np.ndarray) -> np.ndarray:
    """The C oracle on x (a pool, or a flat case's whole signal)."""
    frac, acc, _ = MODES[c.mode]
    return c_oracle().fir1d_rows(x, np.asarray(taps(c)), frac, acc, c.stage)


# ---- the case tables -------------------------------------------------------------------------------------
_PAIRS = (("fast", "acc24"), ("acc24", "wrap32"), ("wrap32", "fast"))

# 3a.  fir1d_mfma_step_kernel<InT, STAGE, KS, ...>: (u8 | int16) x (u8 | int32 out) x KS 2 | 3.  20 taps
# are 2 k-steps and 64 are 3.  int16 -> int32 has no KS 2 form that launches: it takes the matrix
# cores from kMfmaMinTapsI32 = 40 taps on and two k-steps end at 33 (census_cases.UNREACHED), so 40
# taps, its shortest filter, stand in: seven forms, eight filters.
STEP_FORMS = [("u8", U8, 20), ("u8", U8, 64), ("u8", I32, 20), ("u8", I32, 64),
              ("i16", U8, 20), ("i16", U8, 64), ("i16", I32, 40), ("i16", I32, 64)]


def _step_cases():
    out = []
    for i, (dtype, stage, L) in enumerate(STEP_FORMS):
        for mode in _PAIRS[i % 3]:
            out += [Case("step", dtype, stage, L, shape, mode) for shape in ("narrow", "ragged")]
            if L == 64:
                out.append(Case("step", dtype, stage, L, "full", mode))
    return out + [Case("step", "u8", U8, 64, "flat", "fast")]


# 3b.  fir1d_mfma_run_kernel: one L per pipeline configuration (what differs in the loop, by L:
#   66 NS 4, 4 waves per SIMD with u8 out and 3 with int32 out, B re-biased per read; 194 NS 8, windows
#   re-biased in LDS; 290 NS 11, 3 waves; 450 NS 16, 2 waves, int32 out's last one-chunk length; 720
#   u8 out NS 24, the TRIM form, int32 out chunks of 12 in 2-tile runs; 800 u8 out NS 26, 1 wave; 1000
#   u8 out chunks of 6 in 4-tile runs at depth 1, int32 out chunks of 12; 2658 chunks of 8, both stages)
RUN_L = (66, 194, 290, 450, 720, 800, 1000, 2658)
HIGH_PLANE_L = 386
# filter of _mixed_plane_filters -> the HN it takes at HIGH_PLANE_L (test_mfma_sweep_cases.py holds
# them against _high_plane_form; sinc's centre lobe keeps 4 k-steps there)
HIGH_PLANE = {"smooth": 0, "spike_mid": 2, "sinc": 4}


def _run_cases():
    out, k = [], 0
    for L in RUN_L:
        for stage in (U8, I32):
            for mode in ("wrap32", ("fast", "acc24")[k % 2]):
                out += [Case("run", "u8", stage, L, shape, mode) for shape in ("narrow", "full")]
            k += 1
    for filt, hn in HIGH_PLANE.items():
        out += [Case("run", "u8", U8, HIGH_PLANE_L, shape, "fast", filt, hn) for shape in ("narrow", "full")]
    return out + [Case("run", "u8", U8, 66, "flat", "fast")]


# 3c.  fir1d_mfma_long_kernel: int16, chunks of kMlChunk = 16 k-steps.  66 and 257 taps are 4 and 9
# k-steps, one chunk; 483 are 17, two chunks with a last one of a single k-step; 1000 are 33, three.
LONG_L = (66, 257, 483, 1000)
LONG_CHUNKS = {66: (4,), 257: (9,), 483: (16, 1), 1000: (16, 16, 1)}


def long_chunks(L: int) -> tuple:
    """The k-steps of each chunk the chunked kernel walks for L taps."""
    ks = k_steps(L)
    return tuple(min(LONG_CHUNK, ks - s0) for s0 in range(0, ks, LONG_CHUNK))


def _long_cases():
    return [Case("long", "i16", stage, L, shape, mode) for L in LONG_L for stage in (U8, I32)
            for shape in ("narrow", "full") for mode in ("wrap32", "acc24")]


STEP_CASES, RUN_CASES, LONG_CASES = _step_cases(), _run_cases(), _long_cases()
CASES = STEP_CASES + RUN_CASES + LONG_CASES
