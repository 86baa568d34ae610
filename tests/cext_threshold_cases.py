"""The shared route predicates of the complex-rate FIR libraries at their thresholds -- the cases and
references of tests/test_gpu_cext_thresholds.py; a test helper, not a test module.  No GPU.

libfir_cdecim.so, libfir_cinterp.so, libfir_cresample.so and libfir_cstream.so each compile their own
copy of csrc_cext/cext_launch.h's two exactness tests:

* ``needs_wide`` (acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768 >= 2^63): the 64-bit generic
  kernel below the bound, the 128-bit one from it.  ``wide_case`` builds, per library, two tap sets
  whose sum is 2^48 - 1 (accept side: GENERIC64) and 2^48 (reject side: GENERIC128) and a row of
  -32768 samples, so that the outputs whose whole window lies on such samples sum to exactly
  2^63 - 32768 and 2^63: the largest sum 64 bits hold and the first they do not.  2^16 + 1 complex
  taps carry that sum (parts up to 2^31 - 1).  Signs: hr <= 0 and hi >= 0 (variant "re": the real
  part re = sum hr xr - hi xi reaches +sum * 32768) or hr <= 0 and hi <= 0 (variant "im": im = sum
  hr xi + hi xr does).  Where a library interpolates by U the non-zero taps all sit in ONE polyphase
  branch, k = p (mod U): an output of that branch meets all of them, the others none.
* ``dot2_ok`` (every tap part in [-32767, 32767], acc_bits <= 32, frac_bits <= 31): the v_dot2 routes
  (FAST, GENERIC32) inside it, GENERIC64 outside.  ``dot2_pairs`` gives the four boundary pairs.

One model serves all four libraries, their contracts' own (include/fir_c*.h): a row R of frames (x;
x zero-stuffed by U; a stream's hist ++ x), the full-rate complex-tap FIR over R with zeros outside
it, centre c = taps // 2, and kept output m at frame ``idx(m)`` of that filter.  ``exact_sums`` are
those sums as Python ints: every tap part is split into 16-bit halves so that each int64 partial sum
stays below 2^49 (2^16 + 1 products below 2^31 ... 2^32), the halves are joined as Python ints.
``staged`` applies the reference's wrap, rounding and stage to them (test_gpu_range_proofs.py's
_exact_stage); ``oracle_kept`` is the libraries' usual reference -- the committed C oracle over
tests/cplx_ref.py's two real tap sets, what ``want`` of every tests/c*_cases.py computes -- for the
compared outputs alone, the rest of the row passed as the oracle's halos: ``want`` itself filters the
whole row at full rate, 8 * frames * taps = 4 * 10^10 multiplications and more per call here, and
even the run of 1024 kept outputs costs the oracle seconds per call, so ``oracle_spots`` asks it for
three short runs of them (both row ends and the middle).
tests/test_cext_threshold_cases.py holds ``oracle_kept`` against ``want`` where both are cheap.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import cdecim_cases
import cinterp_cases
import cplx_ref
import cresample_cases
import cstream_cases
from oracle import c_oracle

U8, I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)
LIBS = ("cdecim", "cinterp", "cresample", "cstream")
HELPER = {"cdecim": cdecim_cases, "cinterp": cinterp_cases, "cresample": cresample_cases, "cstream": cstream_cases}
RATES = {"cdecim": (1, 2, 1), "cinterp": (2, 1, 0), "cresample": (2, 3, 2), "cstream": (1, 3, 2)}  # U, D, phase
WIDE_STAGES = ((12, 64, U8), (12, 65, U8), (40, 65, I32), (40, 100, I32))  # (frac, acc, stage) of the GPU test
N_WIDE = (1 << 16) + 1   # complex taps that carry a sum of 2^48
PART_MAX = (1 << 31) - 1
BRANCH = 1               # p: the polyphase branch that holds the taps where U > 1
COMPARED = 1024          # kept outputs compared per case, about
MARGIN = 32              # ... of which so many on either side have part of their window outside the row
ENDS = 64                # frames at either end of the row among which the samples that are not -32768 lie


def rate_args(lib: str) -> tuple:
    """The rate arguments of the library's entry, route query and predicted_route, in their order."""
    U, D, phase = RATES[lib]
    return {"cdecim": (D, phase), "cinterp": (U,), "cresample": (U, D, phase), "cstream": (D, phase)}[lib]


def addrs_of(lib: str, x: int, y: int, hist_in: int = 0, hist_out: int = 0) -> tuple:
    """The address arguments of the library's route query: x and y, a stream's two histories between them."""
    return (x, hist_in, y, hist_out) if lib == "cstream" else (x, y)


def predicted(lib: str, addrs: tuple, rows: int, width: int, hq, frac: int, acc: int, stage: int) -> tuple:
    """(route, bucket) by the helper of the library's own GPU test (tests/c*_cases.py's predicted_route)."""
    return HELPER[lib].predicted_route(*addrs, rows, width, hq, *rate_args(lib), frac, acc, stage)


# ---- the model ---------------------------------------------------------------------------------------
def model_row(lib: str, x: np.ndarray, hist: np.ndarray | None) -> np.ndarray:
    """R as (frames, 2) int64: one row x of 2 * width values, stuffed by the library's U, behind hist."""
    U = RATES[lib][0]
    f = np.asarray(x, np.int64).reshape(-1, 2)
    if lib == "cstream":
        return np.concatenate([np.asarray(hist, np.int64).reshape(-1, 2), f])
    R = np.zeros((f.shape[0] * U, 2), np.int64)
    R[::U] = f
    return R


def model_index(lib: str, taps: int, m) -> np.ndarray:
    """idx(m): the frame of the full-rate filter over R that kept output m is."""
    _, D, phase = RATES[lib]
    m = np.asarray(m, np.int64)
    return m * D + phase + ((taps - 1) - taps // 2 if lib == "cstream" else 0)


def exact_sums(R: np.ndarray, hq: np.ndarray, idx) -> tuple[list, np.ndarray]:
    """([(re, im)] as Python ints, pure) for the output frames idx of the full-rate filter over R:
    re = sum_k hr[k] R[i + c - k, 0] - hi[k] R[i + c - k, 1], im = sum_k hr[k] R[.., 1] + hi[k] R[.., 0]
    over the frames inside R.  Zero taps are skipped.  pure[j]: output j meets a non-zero tap, and every
    frame a non-zero tap of it meets is (-32768, -32768)."""
    h = np.asarray(hq, np.int64).reshape(-1, 2)
    L, c = h.shape[0], h.shape[0] // 2
    K = np.flatnonzero((h != 0).any(axis=1))
    assert K.size and np.abs(h).max() <= PART_MAX and np.abs(R).max() <= 32768
    # 16-bit halves: h = (hi16 << 16) + lo16, 0 <= lo16 < 2^16, |hi16| <= 2^15; a partial sum of K.size
    # products of a sample and a half stays below K.size * 2^15 * 2^16
    assert K.size * (1 << 31) < 1 << 49
    G = np.stack([h[K, 0] & 0xFFFF, h[K, 0] >> 16, h[K, 1] & 0xFFFF, h[K, 1] >> 16], axis=1)  # (n, 4)
    pad = L
    Rp = np.zeros((R.shape[0] + 2 * pad, 2), np.int64)
    Rp[pad:pad + R.shape[0]] = R
    step = int(K[1] - K[0]) if K.size > 1 and (np.diff(K) == K[1] - K[0]).all() else 0  # evenly spaced taps: a slice
    sums, pure = [], []
    for i in (int(v) for v in np.asarray(idx).reshape(-1)):
        assert 0 <= i < R.shape[0]
        top = i + c + pad                # tap k meets Rp[top - k]: zeros outside R
        w = Rp[top - K[-1]:top - K[0] + 1:step][::-1] if step else Rp[top - K]  # (n, 2)
        s = np.ascontiguousarray(w.T) @ G  # (2, 4) int64: rows xr, xi; columns hr lo, hr hi, hi lo, hi hi
        rr, ri, ir, ii = ((int(s[a, b + 1]) << 16) + int(s[a, b]) for a, b in ((0, 0), (0, 2), (1, 0), (1, 2)))
        sums.append((rr - ii, ir + ri))  # hr.xr - hi.xi, hr.xi + hi.xr
        pure.append(bool((w == -32768).all()))
    return sums, np.array(pure)


def exact_stage(S: int, frac: int, acc: int, stage: int) -> int:
    """The reference's arithmetic on a Python int (test_gpu_range_proofs.py's _exact_stage): mask to
    acc bits, restore the sign, add the half, shift, saturate (or keep the low 32 bits)."""
    S &= (1 << acc) - 1
    if S & (1 << (acc - 1)):
        S -= 1 << acc
    v = (S + (1 << (frac - 1))) >> frac
    return min(max(v, 0), 255) if stage == U8 else ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def staged(sums, frac: int, acc: int, stage: int) -> np.ndarray:
    """(outputs, 2) of the entry's dtype from exact_sums' sums."""
    out = [[exact_stage(re, frac, acc, stage), exact_stage(im, frac, acc, stage)] for re, im in sums]
    return np.array(out, np.uint8 if stage == U8 else np.int32).reshape(-1, 2)


def oracle_kept(R: np.ndarray, hq, idx, frac: int, acc: int, stage: int) -> np.ndarray:
    """(outputs, 2): the libraries' usual reference for the output frames idx alone.  cplx_ref.want's
    identity (two real filters over R read as 2 * frames real samples, re at the even and im at the
    odd outputs), run by the committed C oracle over the run of frames from the first to the last of
    idx, the rest of R (and the zeros outside it) passed as the oracle's halos."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    lo, hi = int(idx.min()), int(idx.max()) + 1
    g_re, g_im = cplx_ref.as_real_taps(hq)
    G = g_re.size
    HL, HR = G - 1 - G // 2, G // 2
    real = np.zeros(HL + 2 * R.shape[0] + HR, np.int16)
    real[HL:HL + 2 * R.shape[0]] = R.reshape(-1)
    seg = real[HL + 2 * lo:HL + 2 * hi]
    left, right = real[2 * lo:HL + 2 * lo], real[HL + 2 * hi:HL + 2 * hi + HR]
    o = c_oracle()
    re = o.fir1d_rows(seg, g_re, frac, acc, stage, channels=1, halo_left=left, halo_right=right).reshape(-1)[0::2]
    im = o.fir1d_rows(seg, g_im, frac, acc, stage, channels=1, halo_left=left, halo_right=right).reshape(-1)[1::2]
    return np.stack([re[idx - lo], im[idx - lo]], axis=1)


# ---- needs_wide ----------------------------------------------------------------------------------------
@dataclass
class WideCase:
    """One call at the needs_wide threshold.  x: (1, 2 * width); hist: (1, 2 * H) for the stream, else
    None; outputs: the kept outputs that are compared; sums: their exact (re, im); pure: which of them
    have their whole window on -32768 samples; target: the sum those reach in the variant's part."""
    lib: str
    variant: str
    side: str
    hq: np.ndarray
    x: np.ndarray
    hist: np.ndarray | None
    outputs: np.ndarray
    sums: list = field(repr=False)
    pure: np.ndarray = field(repr=False)
    target: int = 0

    @property
    def width(self) -> int:
        return self.x.shape[1] // 2

    @property
    def route(self) -> int:
        return GENERIC64 if self.side == "accept" else GENERIC128

    @property
    def name(self) -> str:
        return f"{self.lib}-{self.variant}-{self.side}"


def wide_taps(lib: str, variant: str, side: str) -> np.ndarray:
    """(taps, 2) int64: N_WIDE non-zero taps at k = p + U t (p = BRANCH where U > 1), nothing after the
    last of them; sum (|hr| + |hi|) = 2^48 - 1 (accept) or 2^48 (reject); rc.wide_case()'s construction
    over two parts a tap: parts of 2^31 - 1, the last tap making up the sum."""
    U = RATES[lib][0]
    p = BRANCH if U > 1 else 0
    total = (1 << 48) - (1 if side == "accept" else 0)
    mag = np.full((N_WIDE, 2), PART_MAX, np.int64)
    rest = total - 2 * (N_WIDE - 1) * PART_MAX   # 2^17 (- 1): what the last tap's two parts must sum to
    mag[-1] = (rest // 2, rest - rest // 2)
    assert int(mag.sum()) == total and mag.max() <= PART_MAX and mag.min() > 0
    mag[:, 0] *= -1                               # hr <= 0
    if variant == "im":
        mag[:, 1] *= -1                           # hi <= 0: im reaches +sum * 32768; else hi >= 0: re does
    hq = np.zeros((p + U * (N_WIDE - 1) + 1, 2), np.int64)
    hq[p::U] = mag
    return hq


_WIDE: dict = {}


def wide_case(lib: str, variant: str, side: str) -> WideCase:
    """The case, built once (the exact sums take about a second)."""
    key = (lib, variant, side)
    if key in _WIDE:
        return _WIDE[key]
    U, D, phase = RATES[lib]
    hq = wide_taps(lib, variant, side)
    L, c = hq.shape[0], hq.shape[0] // 2
    H = L - 1
    rng = np.random.default_rng(sum(map(ord, lib + variant)))  # the two sides of a pair share their samples
    # stuffed frames the model row must have for about COMPARED - 2 MARGIN outputs with a whole window
    # inside it (the stream: every output has one, in the history)
    want_full = (COMPARED - 2 * MARGIN) * D
    if lib == "cstream":
        width = COMPARED * D + 1
    else:
        width = -(-(U * (N_WIDE - 1) + want_full) // U)
    x = np.full((1, 2 * width), -32768, np.int16)
    hist = np.full((1, 2 * H), -32768, np.int16) if lib == "cstream" else None
    left = hist if hist is not None else x        # the row's first frames: the oldest history of a stream
    left[0, rng.integers(0, 2 * ENDS, 40)] = rng.integers(-32768, 32768, 40)
    x[0, 2 * width - 1 - rng.integers(0, 2 * ENDS, 40)] = rng.integers(-32768, 32768, 40)
    R = model_row(lib, x, hist)
    ow = HELPER[lib].out_width(width, *rate_args(lib)) if lib != "cinterp" else width * U
    idx_all = model_index(lib, L, np.arange(ow))
    # outputs whose taps' frames all lie in R: lowest frame idx + c - (L - 1) >= 0, highest idx + c - p < frames
    p = BRANCH if U > 1 else 0
    full = np.flatnonzero((idx_all + c - (L - 1) >= 0) & (idx_all + c - p < R.shape[0]))
    assert full.size, (lib, width)
    outputs = np.arange(max(0, int(full[0]) - MARGIN), min(ow, int(full[-1]) + 1 + MARGIN))
    sums, pure = exact_sums(R, hq, idx_all[outputs])
    target = (1 << 63) - (32768 if side == "accept" else 0)
    _WIDE[key] = WideCase(lib, variant, side, hq, x, hist, outputs, sums, pure, target)
    return _WIDE[key]


def oracle_runs(n: int) -> list:
    """Positions among n compared outputs where the C oracle is asked as well: the first and the last
    24 (windows partly outside the row, the samples that are not -32768) and 48 in the middle (whole
    windows on -32768).  Its cost goes with the frames from the first to the last output of a run
    times the taps (about 3 * 10^8 multiplications for 100 outputs here, in one thread), so not all."""
    return [np.arange(0, 24), np.arange(n // 2 - 24, n // 2 + 24), np.arange(n - 24, n)]


def oracle_spots(w: WideCase, frac: int, acc: int, stage: int) -> tuple[np.ndarray, np.ndarray]:
    """(positions among w.outputs, their (re, im) by oracle_kept), run by run."""
    R = model_row(w.lib, w.x, w.hist)
    idx = model_index(w.lib, w.hq.shape[0], w.outputs)
    runs_ = oracle_runs(w.outputs.size)
    return np.concatenate(runs_), np.concatenate([oracle_kept(R, w.hq, idx[r], frac, acc, stage) for r in runs_])


def wide_ids() -> list:
    return [(lib, variant, side) for lib in LIBS for variant in ("re", "im") for side in ("accept", "reject")]


# ---- dot2_ok -------------------------------------------------------------------------------------------
DOT2_TAPS = 16
DOT2_SHAPES = ((4, 1028), (3, 1030))  # rows of 4 k frames: the fast route takes them; of 4 k + 2: only the generic one


def runs(rng, rows: int, width: int) -> np.ndarray:
    """Samples of +-32767 / -32768 in runs of random lengths (test_wrap_and_rounding_at_the_ends_of_int16's)."""
    ends = np.array([32767, -32768, -32767], np.int16)
    n = rows * 2 * width
    return np.repeat(ends[rng.integers(0, 3, n)], rng.integers(1, 9, n))[:n].reshape(rows, 2 * width).copy()


def dot2_pairs(rng) -> list:
    """[(name, (hq, frac, acc) that stays on a v_dot2 route, (hq, frac, acc) that falls to GENERIC64)]:
    the four neighbours of dot2_ok's limits, every other tap part +-32767."""
    def base():
        return np.where(rng.integers(0, 2, (DOT2_TAPS, 2)) == 0, 32767, -32767).astype(np.int64)

    def poked(k, tap):
        h = base()
        h[k] = tap
        return h

    h1, h2, h3, h4 = base(), base(), base(), base()
    k = DOT2_TAPS // 3
    return [("+32767 | +32768", (poked(k, (32767, -32767)), 12, 32), (poked(k, (32768, 0)), 12, 32)),
            ("-32767 | -32768", (poked(k + 1, (0, -32767)), 12, 32), (poked(k + 1, (0, -32768)), 12, 32)),
            ("acc 32 | 33", (h1, 12, 32), (h2, 12, 33)),
            ("frac 31 | 32", (h3, 31, 32), (h4, 32, 32))]


def reference(lib: str, x: np.ndarray, hist, hq, frac: int, acc: int, stage: int = I32):
    """The library's own reference: (y, hist_out or None)."""
    a = rate_args(lib)
    if lib == "cstream":
        y, hist_out, _ = cstream_cases.want_block(x, hist, hq, *a, frac, acc, stage)
        return y, hist_out
    return HELPER[lib].want(x, hq, *a, frac, acc, stage), None
