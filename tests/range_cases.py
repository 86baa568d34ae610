"""Threshold cases for the host-side range proofs that pick the narrow kernel forms.

Three parts (tests/test_range_cases.py checks this module on the CPU, tests/test_gpu_range_proofs.py
runs its cases on the GPU against the C oracle):

1. worst-case inputs: periodic u8 / int16 rows and u8 frames whose interior outputs attain the
   exact extremes of sum_k h[k] x[n - k + c] (``worst_rows_u8``, ``worst_rows_i16``,
   ``worst_frames_u8``), plus all-0, all-255, uniform random and random-from-the-two-ends rows;
2. tap builders with a prescribed sum of positive taps, sum of negative taps, common power of two
   and largest tap (``taps_1d``, ``taps_2d``, ``outer``);
3. ``CASES``: per predicate of the sources (restated here in Python, cited by file and line) a pair
   of configurations, the last one the proof accepts and the first it rejects, differing by one
   unit (``Case.unit``) in one tap, or, for the few predicates on frac_bits, by one in frac_bits.
   Where the narrow form is still right just past the proof (the proof is conservative), a third
   configuration ``extra`` is the first at which the narrow form breaks.  ``Case.narrow`` is a
   few-line model of the narrow form; test_range_cases.py asserts that it differs from the oracle
   on the worst-case input of ``reject`` or ``extra`` for every case, so no case is vacuous.
   ``SEAMS`` lists dispatch seams whose two sides compute the same values in either form
   (frac_bits limits, the clamp of the shift at frac - 1): both sides run on the GPU, nothing more.

Not covered, on purpose: the 128-bit threshold (needs_wide, fir1d.hip:159; wide, fir2d.hip:296)
for u8 samples.  255 sum|h| reaches 2^63 only from about 1.7e7 taps of 2^31 - 1, and an output
attains the bound only in a row (a frame) at least as large as the filter.  The int16 1-D
threshold (2^17 taps) is wide_case().  One bound of launch2d_reg cannot be reached either: the
register path wants int16 taps (fir2d.hip:305), so a column factor is at most 32768 in magnitude
and the test |col| < 2^23 (fir2d.hip:164) never fails.  (col <= 32767, fir2d.hip:179, does: a tap
of -32768 over a row tap of -1 is a column factor of +32768.)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Callable

import numpy as np

from oracle import fir_oracle as fo

U8, I32 = fo.OUT_U8_SAT, fo.OUT_I32


# ---- 1. worst-case inputs ------------------------------------------------------------------
def _seed(h) -> int:
    return int(np.abs(np.asarray(h, np.int64)).sum() % (1 << 31)) + np.asarray(h).size


def _pattern(hq, hi, lo, zero):
    """One period of the row that attains the high extreme: hi under h > 0, lo under h < 0."""
    h = np.asarray(hq, np.int64)
    L, c = h.size, h.size // 2
    pat = np.full(L, zero, np.int64)
    for k in range(L):
        if h[k] != 0:
            pat[(c - k) % L] = hi if h[k] > 0 else lo
    return pat


def _periodic_rows(hq, width, phases, hi, lo, zero_hi, zero_lo):
    L = np.asarray(hq).size
    i = np.arange(width)
    rows, names = [], []
    for p in range(min(L, phases)):
        rows.append(_pattern(hq, hi, lo, zero_hi)[(i - p) % L])
        names.append(f"high+{p}")
        rows.append(_pattern(hq, lo, hi, zero_lo)[(i - p) % L])
        names.append(f"low+{p}")
    return rows, names


def worst_rows_u8(hq, width: int, phases: int = 16):
    """(rows, names): per phase p < min(L, phases) a row whose outputs n = p (mod L) attain
    255 sum(h > 0) and one whose outputs attain 255 sum(h < 0), in the row's interior; then all-0,
    all-255, uniform random and random-from-{0, 255} rows."""
    rows, names = _periodic_rows(hq, width, phases, 255, 0, 0, 255)
    rng = np.random.default_rng(_seed(hq))
    rows += [np.zeros(width, np.int64), np.full(width, 255), rng.integers(0, 256, width),
             rng.choice(np.array([0, 255]), width)]
    names += ["zeros", "full", "random", "random_ends"]
    return np.stack(rows).astype(np.uint8), names


def worst_rows_i16(hq, width: int, phases: int = 16):
    """As worst_rows_u8 with 32767 / -32768 under the taps by sign (each arrangement: the high rows
    hold 32767 under h > 0 and -32768 under h < 0, the low rows the reverse), rows of -32768 and
    of 32767 alone, and each phase-0 row again with the sample under the smallest tap one unit
    nearer zero (a sum one tap short of the extreme)."""
    h = np.asarray(hq, np.int64)
    L, c = h.size, h.size // 2
    rows, names = _periodic_rows(h, width, phases, 32767, -32768, 0, 0)
    ks = np.flatnonzero(h)
    if ks.size:
        k = int(ks[np.argmin(np.abs(h[ks]))])
        for r, name in ((0, "high"), (1, "low")):
            near = rows[r].copy()
            at = np.arange((c - k) % L, width, L)
            near[at] -= np.sign(near[at])
            rows.append(near)
            names.append(name + "_near")
    rng = np.random.default_rng(_seed(h))
    rows += [np.zeros(width, np.int64), np.full(width, -32768), np.full(width, 32767),
             rng.integers(-32768, 32768, width), rng.choice(np.array([-32768, 32767]), width)]
    names += ["zeros", "min", "max", "random", "random_ends"]
    return np.stack(rows).astype(np.int16), names


def worst_frames_u8(hq2, H: int, W: int, phases: int = 9):
    """(frames, names): frames of period (R, C) that attain 255 sum(h > 0) / 255 sum(h < 0) at
    the interior pixels (i, j) = (dy, dx) (mod (R, C)), for the first ``phases`` shifts (dy, dx)
    in column-fastest order, then all-0, all-255, uniform random and random-from-{0, 255} frames."""
    h = np.asarray(hq2, np.int64)
    R, C = h.shape
    cr, cc = R // 2, C // 2
    hi = np.zeros((R, C), np.int64)
    lo = np.zeros((R, C), np.int64)
    for m in range(R):
        for n in range(C):
            hi[(cr - m) % R, (cc - n) % C] = 255 if h[m, n] > 0 else 0
            lo[(cr - m) % R, (cc - n) % C] = 255 if h[m, n] < 0 else 0
    ii, jj = np.arange(H)[:, None], np.arange(W)[None, :]
    frames, names = [], []
    for p in range(min(R * C, phases)):
        dy, dx = (p // C) % R, p % C
        frames.append(hi[(ii - dy) % R, (jj - dx) % C])
        names.append(f"high+{dy},{dx}")
        frames.append(lo[(ii - dy) % R, (jj - dx) % C])
        names.append(f"low+{dy},{dx}")
    rng = np.random.default_rng(_seed(h))
    frames += [np.zeros((H, W), np.int64), np.full((H, W), 255), rng.integers(0, 256, (H, W)),
               rng.choice(np.array([0, 255]), (H, W))]
    names += ["zeros", "full", "random", "random_ends"]
    return np.stack(frames).astype(np.uint8), names


def mac2d(x, hq2) -> np.ndarray:
    """The exact 2-D sums, through fir2d_fixed at a stage that exposes them: taps doubled,
    frac_bits = 1, no wrap: ((2 S) + 1) >> 1 == S (|S| < 2^31 for u8 frames and int16 taps)."""
    return fo.fir2d_fixed(x, 2 * np.asarray(hq2, np.int64), 1, 64, I32).astype(np.int64)


# ---- 2. tap builders -----------------------------------------------------------------------
def _spread(total: int, slots: int, first) -> list:
    if slots == 0:
        assert total == 0
        return []
    if first is not None:
        assert slots >= 2 and total > first
        return [first] + _spread(total - first, slots - 1, None)
    return [total // slots + (1 if i < total % slots else 0) for i in range(slots)]


def taps_1d(L: int, pos: int, neg: int = 0, s: int = 0, hmax: int | None = None, first: int | None = None,
            sign: int = 1) -> np.ndarray:
    """L taps h = sign * 2^s * h' with sum(h' > 0) == pos, sum(h' < 0) == -neg, h' not all even
    (2^s is exactly the taps' common power of two) and max |h| <= hmax.  Positive h' sit on the
    even indices (all indices when neg == 0, or the odd ones when pos == 0), negative ones on the
    others; ``first`` fixes the first positive h' (a small tap beside large ones)."""
    if neg == 0:
        pi, ni = list(range(L)), []
    elif pos == 0:
        pi, ni = [], list(range(L))
    else:
        pi, ni = list(range(0, L, 2)), list(range(1, L, 2))
    hp = np.zeros(L, np.int64)
    hp[pi] = _spread(pos, len(pi), first)
    hp[ni] = [-v for v in _spread(neg, len(ni), None)]
    if not (hp % 2).any():  # move one unit between two taps of one sign: the sums stay
        idx = pi if len(pi) >= 2 else ni
        assert len(idx) >= 2 and abs(hp[idx[-1]]) > 1, "cannot make the taps' odd part odd"
        sg = 1 if idx is pi else -1
        hp[idx[0]] += sg
        hp[idx[-1]] -= sg
    h = sign * (hp << s)
    assert int(hp[hp > 0].sum()) == pos and int(-hp[hp < 0].sum()) == neg and (hp % 2).any()
    assert hmax is None or int(np.abs(h).max()) <= hmax, (int(np.abs(h).max()), hmax)
    return h


def is_rank1(h2) -> bool:
    h = [[int(v) for v in r] for r in np.asarray(h2)]
    R, C = len(h), len(h[0])
    return all(h[a][b] * h[m][n] == h[a][n] * h[m][b] for a in range(R) for m in range(a + 1, R)
               for b in range(C) for n in range(b + 1, C))


def taps_2d(R: int, C: int, pos: int, neg: int = 0, s: int = 0, hmax: int | None = None, sign: int = 1) -> np.ndarray:
    """An (R, C) tap set as taps_1d builds it (row-major), guaranteed NOT rank-1: while it is, one
    unit of h' moves between two positive (or two negative) taps."""
    h = taps_1d(R * C, pos, neg, s, hmax, sign=sign).reshape(R, C)
    idx = [tuple(i) for i in np.argwhere(h * sign > 0)] if pos else [tuple(i) for i in np.argwhere(h != 0)]
    step = sign * (1 << s) * (1 if pos else -1)
    for a in range(len(idx) - 1):
        if not is_rank1(h):
            break
        if abs(h[idx[a + 1]]) > 2 * abs(step):
            h[idx[a]] += 2 * step  # two units: the odd part of one of the taps stays odd
            h[idx[a + 1]] -= 2 * step
    assert not is_rank1(h)
    assert hmax is None or int(np.abs(h).max()) <= hmax
    return h


def outer(col, row) -> np.ndarray:
    """The rank-1 set col[m] * row[n]."""
    return np.outer(np.asarray(col, np.int64), np.asarray(row, np.int64))


# ---- the predicates, restated --------------------------------------------------------------
def habs(h) -> int:
    return int(np.abs(np.asarray(h, np.int64)).sum())


def psum(h) -> int:
    h = np.asarray(h, np.int64)
    return int(h[h > 0].sum())


def nsum(h) -> int:
    h = np.asarray(h, np.int64)
    return int(h[h < 0].sum())


def taps16(h) -> bool:
    """fir1d_reg_impl.h:165-166, fir2d.hip:304-305."""
    h = np.asarray(h, np.int64)
    return bool(h.min() >= -32768 and h.max() <= 32767)


def nowrap(h, frac: int, acc: int, xmax: int = 255) -> bool:
    """fir1d_reg_impl.h:169-174 (per filter), fir2d.hip:155-157, fir1d_mfma.hip:1032-1033
    (xmax = 32768 for int16 samples): no sum plus the rounding half reaches 2^(acc-1)."""
    return frac <= 22 and xmax * habs(h) + (1 << (frac - 1)) < (1 << (acc - 1))


def u8dot2(bank, frac: int, acc: int) -> bool:
    """fir1d_reg_impl.h:182: the byte-pair v_dot2 form: int16 taps and no filter can wrap."""
    bank = np.atleast_2d(np.asarray(bank, np.int64))
    return taps16(bank) and all(nowrap(h, frac, acc) for h in bank)


def u8_noclamp(h, frac: int) -> bool:
    """fir1d_reg.h:124-129: 2^(f-1) + sum h x in [0, 256 * 2^f) for every u8 x."""
    if not 1 <= frac <= 22:
        return False
    half = 1 << (frac - 1)
    return half + 255 * nsum(h) >= 0 and half + 255 * psum(h) < (256 << frac)


def common_shift(h, frac: int):
    """fir1d_reg.h:143-152, fir2d_reg.h:125-133, fir2d_mfma.hip:358-369: the largest power of two
    common to the non-zero taps, at most frac - 1 (None for all-zero taps)."""
    h = np.asarray(h, np.int64).reshape(-1)
    nz = h[h != 0]
    if nz.size == 0:
        return None
    z = min(int(v & -v).bit_length() - 1 for v in (int(t) for t in nz))
    return min(z, frac - 1)


def pk16_plan(h, frac: int) -> dict:
    """fir1d_reg.h:137-172 for one filter and fir2d_reg.h:123-154 for a general kernel:
    mode 0 (refused), 1 (unsigned V) or 2 (signed V), V = 2^(f-1-s) + sum (h >> s) x."""
    out = {"mode": 0, "s": None, "vmax": None, "vmin": None}
    if not 1 <= frac <= 22:
        return out
    s = common_shift(h, frac)
    if s is None:
        return out
    out["s"] = s
    hp = np.asarray(h, np.int64) >> s
    bias = 1 << (frac - 1 - s)
    out["vmax"], out["vmin"] = bias + 255 * psum(hp), bias + 255 * nsum(hp)
    if frac - s > 15:  # 16-bit shifts take the amount mod 16
        return out
    if out["vmin"] >= 0 and out["vmax"] <= 65535:
        out["mode"] = 1
    elif out["vmin"] >= -32768 and out["vmax"] <= 32767:
        out["mode"] = 2
    return out


def pk16_bank(bank, frac: int, acc: int) -> dict:
    """fir1d_reg_impl.h:175-181 with fir1d_reg.h:168-171: the bank's per-filter modes, whether the
    packed-16 kernel runs at all, and whether every filter is unsigned with shift 8 (hi8)."""
    bank = np.atleast_2d(np.asarray(bank, np.int64))
    plans = [pk16_plan(h, frac) for h in bank]
    modes = [p["mode"] for p in plans] if u8dot2(bank, frac, acc) and len(bank) > 1 else [0] * len(bank)
    hi8 = all(m == 1 and frac - p["s"] == 8 for m, p in zip(modes, plans))
    return {"modes": modes, "pk16": any(modes), "hi8": hi8, "plans": plans}


def mfma1d_taps_ok(h) -> bool:
    """fir1d_mfma.hip:1059-1060: the high byte of the balanced split is a signed byte."""
    h = np.asarray(h, np.int64)
    return bool(h.min() >= -32768 and h.max() <= 32639)


def needs_wide(h, acc: int, xmax: int) -> bool:
    """fir1d.hip:159-165 (xmax = 255 or 32768), fir2d.hip:296-301 (xmax = 255)."""
    return acc >= 64 and habs(h) * xmax >= (1 << 63)


def rank1_factor(h2):
    """fir2d.hip:111-144: (col, row) with h == outer(col, row), row = the first non-zero row of h
    over its gcd (int16), or None."""
    h = [[int(v) for v in r] for r in np.asarray(h2)]
    R, C = len(h), len(h[0])
    nz = [(m, n) for m in range(R) for n in range(C) if h[m][n]]
    if not nz:
        return None
    r0, n0 = nz[0]
    g = functools.reduce(np.gcd, [abs(v) for v in h[r0]])
    row = [v // int(g) for v in h[r0]]
    if min(row) < -32768 or max(row) > 32767:
        return None
    col = []
    for m in range(R):
        if h[m][n0] % row[n0]:
            return None
        a = h[m][n0] // row[n0]
        if any(h[m][n] != a * row[n] for n in range(C)):
            return None
        col.append(a)
    return np.array(col, np.int64), np.array(row, np.int64)


def sep_form(h2, frac: int, acc: int) -> str:
    """fir2d.hip:159-165 and :176-179: "sep16" (int16 row sums), "sep" (24-bit row sums) or
    "general" for a tap set the register path takes."""
    f = rank1_factor(h2)
    R, C = np.asarray(h2).shape
    if f is None or R < 2 or C < 2:
        return "general"
    col, row = f
    if not (255 * habs(row) < (1 << 23) and col.min() >= -(1 << 23) and col.max() < (1 << 23)):
        return "general"
    if 255 * habs(row) <= 32767 and col.min() >= -32768 and col.max() <= 32767:
        return "sep16"
    return "sep"


def pk16_plan_rank1(h2, frac: int) -> dict:
    """fir2d_reg.h:82-118 on the factors of rank1_factor: s = min(zc + zr, f - 1), taken from the
    column factor first (sc = min(s, zc), sr = s - sc)."""
    out = {"mode": 0, "s": None, "sc": None, "sr": None, "vmax": None, "vmin": None}
    f = rank1_factor(h2)
    if f is None or not 1 <= frac <= 22:
        return out
    col, row = f
    zc, zr = common_shift(col, 64), common_shift(row, 64)
    if zc is None or zr is None:
        return out
    s = min(zc + zr, frac - 1)
    sc = min(s, zc)
    sr = s - sc
    out.update(s=s, sc=sc, sr=sr, zc=zc, zr=zr)
    p = outer(col >> sc, row >> sr)
    bias = 1 << (frac - 1 - s)
    out["vmax"], out["vmin"] = bias + 255 * psum(p), bias + 255 * nsum(p)
    if frac - s > 15:
        return out
    if out["vmin"] >= 0 and out["vmax"] <= 65535:
        out["mode"] = 1
    elif out["vmin"] >= -32768 and out["vmax"] <= 32767:
        out["mode"] = 2
    return out


def pk16_2d(h2, frac: int, acc: int) -> dict:
    """fir2d.hip:188-189 / :228-230: the packed-16 plan the register path uses for the u8 stage
    (rank-1 sets that pass the separable test: plan_pk16, every other: plan_pk16_gen)."""
    if not nowrap(h2, frac, acc):
        return {"mode": 0, "s": None, "vmax": None, "vmin": None}
    return pk16_plan_rank1(h2, frac) if sep_form(h2, frac, acc) != "general" else pk16_plan(h2, frac)


def mfma2_plan(h2, frac: int, acc: int) -> dict:
    """fir2d_mfma.hip:355-401: np = 0 (refused), 1 (taps >> s are signed bytes) or 2 (balanced
    byte pairs); fast: the rounded sum, shifted so that its byte sits in bits 16..23, fits int32."""
    R, C = np.asarray(h2).shape
    if R not in (3, 5) or C > 5 or not 1 <= frac <= 31 or acc > 32:  # launch_fir2d_mfma: R in {3, 5}
        return {"np": 0, "fast": False, "s": None}
    s = common_shift(h2, frac)
    s = 0 if s is None else s
    v = np.asarray(h2, np.int64) >> s
    if v.min() < -32768 or v.max() > 32639:
        return {"np": 0, "fast": False, "s": s}
    planes = 1 if v.min() >= -128 and v.max() <= 127 else 2
    top = 255 * habs(h2) + (1 << (frac - 1))
    fast = top < (1 << (acc - 1)) and frac <= 16 and (top << (16 - frac) if frac <= 16 else 0) < (1 << 31)
    return {"np": planes, "fast": bool(fast), "s": s}


# ---- narrow-form models --------------------------------------------------------------------
def _wrap(v, bits: int):
    v = np.asarray(v, np.int64)
    m = np.int64(1) << np.int64(bits)
    return ((v + (m >> np.int64(1))) & (m - np.int64(1))) - (m >> np.int64(1))


def _stage(q, stage: int):
    return fo._stage(np.asarray(q, np.int64), stage)


def m_nowrap(S, frac: int, stage: int):
    """The no-wrap forms: the accumulator starts at the rounding half and is never wrapped to
    acc_bits; the hardware's 32 bits hold wrap32(S + half)."""
    return _stage(_wrap(S + (1 << (frac - 1)), 32) >> np.int64(frac), stage)


def m_noclamp(S, frac: int):
    """The u8 stage as a shift alone: the low byte of (S + half) >> frac."""
    return (((S + (1 << (frac - 1))) >> np.int64(frac)) & np.int64(255)).astype(np.uint8)


def m_pk16(S, frac: int, s: int, signed: bool):
    """Packed 16-bit pairs: V = (2^(f-1-s) + S / 2^s) mod 2^16, a 16-bit shift by (f - s) mod 16
    (logical for an unsigned V, arithmetic for a signed one), then the clamp to [0, 255]."""
    V = ((S >> np.int64(s)) + (1 << (frac - 1 - s))) & np.int64(0xFFFF)
    if signed:
        V = _wrap(V, 16)
    return np.clip(V >> np.int64((frac - s) % 16), 0, 255).astype(np.uint8)


def m_hi8(S, frac: int, s: int):
    """Packed 16-bit pairs, every filter unsigned with f - s == 8: the output is V's high byte."""
    V = ((S >> np.int64(s)) + (1 << (frac - 1 - s))) & np.int64(0xFFFF)
    return (V >> np.int64(8)).astype(np.uint8)


def m_taps_int16(h):
    """Taps packed as int16 halves for v_dot2."""
    return _wrap(h, 16)


def m_taps_byte_pair(h):
    """The balanced split v = 256 hi + lo with hi stored as a signed byte."""
    h = np.asarray(h, np.int64)
    lo = _wrap(h, 8)
    return 256 * _wrap((h - lo) // 256, 8) + lo


def m_taps_byte(h, s: int):
    """One signed byte per tap after the common shift."""
    return _wrap(np.asarray(h, np.int64) >> s, 8) << s


def m_sep(x, h2, frac: int, acc: int, stage: int, bits: int, col_bits: int = 64):
    """The separable forms: each input row's sum over the row factor is held in ``bits`` bits
    (16: packed int16 pairs; 24: an operand of the 24-bit multiplier) before the column pass, whose
    taps are held in ``col_bits`` bits (16: packed beside the row sums)."""
    col, row = rank1_factor(h2)
    col = _wrap(col, col_bits) if col_bits < 64 else col
    rs = _wrap(fo._mac_rows(np.asarray(x, np.int64), row), bits)
    S = fo._mac_rows(np.ascontiguousarray(rs.T), col).T
    return _stage(fo.wrap_round(S, frac, acc), stage)


def m_mfma2_fast(S, frac: int):
    """fir2d_mfma.hip's fast form: (S + half) << (16 - f) in 32 bits, the clamped byte of bits 16..23."""
    t = _wrap((S + (1 << (frac - 1))) << np.int64(16 - frac), 32)
    return np.clip(t >> np.int64(16), 0, 255).astype(np.uint8)


# ---- 3. the case table ---------------------------------------------------------------------
@dataclass(frozen=True)
class Side:
    taps: np.ndarray  # (L,), a bank (F, L), or a kernel (R, C)
    frac: int = 12
    acc: int = 32


@dataclass
class Case:
    id: str
    row: str            # the source row of the table in DESIGN.md ("range proofs")
    cite: str           # file:line of the predicate
    kind: str           # "rows" (one filter), "bank" (F filters) or "frame" (2-D)
    accept: Side
    reject: Side
    predicate: Callable  # Side -> bool: the narrow form is taken
    narrow: Callable     # (x, Side, stage) -> the narrow form's output for filter ``f`` of the side
    bounds: Callable     # Side -> (vmax, vmin) as the predicate computes them
    quantity: Callable = lambda S, side: S  # exact sums -> the quantity the predicate bounds
    extra: Side | None = None  # conservative proofs: the first configuration the narrow form fails
    unit: int = 1
    dtype: type = np.uint8
    stages: tuple = (U8, I32)
    f: int = 0           # banks: the filter that crosses
    path: str | None = None  # FIR2D_PATH
    frames2: bool = False  # also one call with a batch of two frames
    # What a call's launch log (fir_hip.launch_log) must show.  form: Launch -> bool, "this is the
    # narrow form the proof admits": every launch of an accept-side call has it, and a reject- or
    # conservative-side call has at least one launch without it.  runtime: the proof picks a field
    # of the tap record that the kernel reads at run time, not an instantiation, so the log cannot
    # tell the sides apart; both sides must then launch `form`, the kernel that reads the field.
    form: Callable | None = None
    runtime: bool = False

    @property
    def tight(self) -> bool:
        return self.extra is None

    def sides(self):
        out = [("accept", self.accept), ("reject", self.reject)]
        return out + ([("conservative", self.extra)] if self.extra is not None else [])

    def filter_taps(self, side: Side) -> np.ndarray:
        return side.taps[self.f] if self.kind == "bank" else side.taps

    def inputs(self, side: Side, shape):
        """(x, names) of the worst-case rows (rows x shape) or frames (n x H x W) for ``side``."""
        h = self.filter_taps(side)
        if self.kind == "frame":
            return worst_frames_u8(h, *shape)
        return (worst_rows_u8 if self.dtype == np.uint8 else worst_rows_i16)(h, shape)

    def sums(self, x, side: Side):
        h = self.filter_taps(side)
        if self.kind == "frame":
            return np.stack([mac2d(f, h) for f in x])
        return fo._mac_rows(np.asarray(x, np.int64), h)

    def oracle(self, x, side: Side, stage: int):
        h = self.filter_taps(side)
        if self.kind == "frame":
            return np.stack([fo.fir2d_fixed(f, h, side.frac, side.acc, stage) for f in x])
        return fo.fir1d_rows(x, h, side.frac, side.acc, stage)


def _one_sided(xmax_pos: int, xmax_neg: int):
    """Bounds of a predicate on sum|h| for taps of one sign."""
    def bounds(side):
        h = np.asarray(side.taps, np.int64)
        a = habs(h)
        return (xmax_pos * a, -xmax_neg * a) if (h >= 0).all() else (xmax_neg * a, -xmax_pos * a)
    return bounds


def _u8_bounds(case_taps=lambda side: side.taps):
    return lambda side: (255 * psum(case_taps(side)), 255 * nsum(case_taps(side)))


CASES: list[Case] = []
SEAMS: list[dict] = []


def _bank_plan(f: int):
    """Side -> the packed-16 plan of filter ``f`` of its bank."""
    return lambda side: pk16_plan(side.taps[f], side.frac)


def _frame_plan(side) -> dict:
    return pk16_2d(side.taps, side.frac, side.acc)


def _pk_bounds(plan):
    """Side -> (vmax, vmin) of V as ``plan`` (Side -> dict) computes them."""
    return lambda side: (plan(side)["vmax"], plan(side)["vmin"])


def _pk_quantity(plan):
    """(exact sums, Side) -> V = 2^(f-1-s) + S / 2^s with the shift of ``plan``."""
    def q(S, side):
        sh = plan(side)["s"]
        return (S >> np.int64(sh)) + (1 << (side.frac - 1 - sh))
    return q


def _bump(h, idx, by):
    h = np.array(h, np.int64)
    h[idx] += by
    return h


def _first_pos(h) -> tuple:
    h = np.asarray(h)
    return tuple(np.argwhere(h > 0)[0]) if (h > 0).any() else tuple(np.argwhere(h < 0)[0])


def _grow(h, by: int = 1):
    """One more unit of |h| on the first positive tap (the first negative one of negative sets)."""
    i = _first_pos(h)
    return _bump(h, i, by if np.asarray(h)[i] > 0 else -by)


def _grow_neg(h, by: int = 1):
    """One more unit of |h| on the first negative tap."""
    return _bump(h, tuple(np.argwhere(np.asarray(h) < 0)[0]), -by)


def _nowrap_case(cid, row, cite, kind, h_accept, frac, acc, steps_to_break, predicate, dtype=np.uint8, xmax=(255, 0),
                 stages=(U8, I32), path=None, f=0, frames2=False):
    """A predicate on sum|h| (the rounding half included): accept = the last set below it, reject =
    one unit more, extra = ``steps_to_break`` units more, the first whose sum alone reaches
    2^(acc-1) (None: the proof is tight)."""
    def grow(h, by):
        if kind != "bank":
            return _grow(h, by)
        h = np.array(h, np.int64)
        h[f] = _grow(h[f], by)
        return h

    c = Case(cid, row, cite, kind, Side(h_accept, frac, acc), Side(grow(h_accept, 1), frac, acc), predicate,
             None, None, dtype=dtype, stages=stages, path=path, f=f, frames2=frames2,
             extra=None if steps_to_break is None else Side(grow(h_accept, steps_to_break), frac, acc))

    def narrow(x, side, stage, c=c):
        return m_nowrap(c.sums(x, side), side.frac, stage)

    def bounds(side, c=c):
        return _one_sided(*xmax)(Side(c.filter_taps(side), side.frac, side.acc))

    c.narrow, c.bounds = narrow, bounds
    CASES.append(c)
    return c


# -- row "launch_reg": fir1d_reg_impl.h:164-192 ----------------------------------------------
_REG = "fir1d_reg_impl.h:165-183"
_p_u8dot2 = lambda side: u8dot2(side.taps, side.frac, side.acc)  # noqa: E731
# 255 * 32888 + 2048 = 8388488 < 2^23 <= 255 * 32889 + 2048; the sum alone reaches 2^23 from 32897
_nowrap_case("reg-nowrap-acc24-f12-pos", "launch_reg", _REG, "rows", taps_1d(3, 32888), 12, 24, 9, _p_u8dot2)
_nowrap_case("reg-nowrap-acc24-f12-neg", "launch_reg", _REG, "rows", taps_1d(9, 32888, sign=-1), 12, 24, 9, _p_u8dot2)
# 255 * 127 + 128 = 32513 < 2^15 <= 255 * 128 + 128; the sum alone reaches 2^15 from 129
_nowrap_case("reg-nowrap-acc16-f8", "launch_reg", _REG, "rows", taps_1d(5, 127), 8, 16, 2, _p_u8dot2)
for _F in (2, 4):  # a bank in which only filter F - 1 crosses
    _bank = np.stack([taps_1d(5, 4000 + 7 * i, 90 * i) for i in range(_F - 1)] + [taps_1d(5, 32888)])
    _nowrap_case(f"reg-nowrap-acc24-bank{_F}", "launch_reg", _REG, "bank", _bank, 12, 24, 9, _p_u8dot2, f=_F - 1)


def _taps16_case(cid, h_accept, idx, by):
    c = Case(cid, "launch_reg", "fir1d_reg_impl.h:165-166", "rows", Side(h_accept), Side(_bump(h_accept, idx, by)),
             _p_u8dot2, lambda x, side, stage: fo.fir1d_rows(x, m_taps_int16(side.taps), side.frac, side.acc, stage),
             _u8_bounds())
    CASES.append(c)


_taps16_case("reg-taps16-32767", np.array([-5, 32767, 40]), 1, 1)
_taps16_case("reg-taps16--32768", np.array([3, -32768, 7, 0, -1]), 1, -1)
SEAMS.append(dict(id="reg-frac22-23", row="launch_reg", cite="fir1d_reg_impl.h:169", kind="rows", dtype=np.uint8,
                  sides=[Side(taps_1d(5, 3000, 2000), 22, 32), Side(taps_1d(5, 3000, 2000), 23, 32)], path=None,
                  stages=(U8, I32), value=lambda s: u8dot2(s.taps, s.frac, s.acc), expect=[True, False],
                  why="nine int16 taps times 255 plus 2^22 stay below 2^31: the no-wrap form is exact at frac 23 too"))

# -- row "plan_u8_noclamp": fir1d_reg.h:124-129 -----------------------------------------------
_p_noclamp = lambda side: u8_noclamp(side.taps, side.frac)  # noqa: E731


def _noclamp_case(cid, h_accept, h_reject, frac):
    c = Case(cid, "plan_u8_noclamp", "fir1d_reg.h:126-128", "rows", Side(h_accept, frac), Side(h_reject, frac),
             _p_noclamp, lambda x, side, stage: m_noclamp(fo._mac_rows(np.asarray(x, np.int64), side.taps), side.frac),
             lambda side: ((1 << (side.frac - 1)) + 255 * psum(side.taps), (1 << (side.frac - 1)) + 255 * nsum(side.taps)),
             quantity=lambda S, side: S + (1 << (side.frac - 1)), stages=(U8,))
    CASES.append(c)


# 255 * 4104 + 2048 = 1048568 < 2^20 <= 255 * 4105 + 2048 (c = 1368 / 1369 of test_bank_noclamp_stage_boundary)
_noclamp_case("noclamp-f12-vmax", np.array([1368, 1368, 1368]), np.array([1368, 1369, 1368]), 12)
_noclamp_case("noclamp-f12-vmax-mixed", taps_1d(5, 4104, 8), _grow(taps_1d(5, 4104, 8)), 12)
# 255 * 256 + 128 = 65408 < 2^16 <= 255 * 257 + 128
_noclamp_case("noclamp-f8-vmax", taps_1d(9, 256), _grow(taps_1d(9, 256)), 8)
# 255 * 32832 + 16384 = 8388544 < 2^23 <= 255 * 32833 + 16384
_noclamp_case("noclamp-f15-vmax", taps_1d(3, 32832), _grow(taps_1d(3, 32832)), 15)
# 2^(f-1) is no multiple of 255, so vmin = 0 cannot be hit: 2048 - 255 * 8 = 8 >= 0 > 2048 - 255 * 9 = -247
_noclamp_case("noclamp-f12-vmin", taps_1d(5, 900, 8), _bump(taps_1d(5, 900, 8), 1, -1), 12)
# 128 - 255 * 0 >= 0 > 128 - 255
_noclamp_case("noclamp-f8-vmin", np.array([20, 0, 30]), np.array([20, -1, 30]), 8)

# -- row "plan_u8_pk16": fir1d_reg.h:137-172 (banks, u8 stage) ---------------------------------
_BENIGN = np.array([0, 0, 1024, 2048, 1024])  # a packed-16 filter (s = 10) beside the one that crosses


def _pk16_1d_case(cid, h_accept, h_reject, frac, want: int, unit=1, benign=_BENIGN):
    """The crossing filter (filter 0 of a bank of two) has packed-16 mode ``want`` on the accept
    side and another mode (0: the v_dot2 form; 2: signed) on the reject side."""
    L = len(h_accept)
    b = np.zeros(L, np.int64)
    b[:min(L, 5)] = benign[-min(L, 5):]

    plan = _bank_plan(0)

    def narrow(x, side, stage):
        S = fo._mac_rows(np.asarray(x, np.int64), side.taps[0])
        return m_pk16(S, side.frac, plan(side)["s"], want == 2)

    def pred(side):
        return pk16_bank(side.taps, side.frac, side.acc)["modes"][0] == want

    CASES.append(Case(cid, "plan_u8_pk16", "fir1d_reg.h:154-161", "bank", Side(np.stack([h_accept, b]), frac),
                      Side(np.stack([h_reject, b]), frac), pred, narrow, _pk_bounds(plan),
                      quantity=_pk_quantity(plan), unit=unit, stages=(U8,)))


def _pk_pair(L, pos, neg, s, grow_pos: bool):
    """taps_1d(L, pos, neg, s) and the same with one more unit 2^s on a tap of the sign to grow (a
    zero tap if growing another would make every h' even)."""
    a = taps_1d(L, pos, neg, s)
    for i in [int(i) for i in np.flatnonzero(a > 0 if grow_pos else a < 0)[::-1]] + [int(i) for i in np.flatnonzero(a == 0)]:
        b = _bump(a, i, (1 << s) if grow_pos else -(1 << s))
        if common_shift(b, 64) == s:
            return a, b
    raise AssertionError("no tap to grow")


# s = 0, frac 12 (bias 2048): unsigned 2048 + 255 * 248 = 65288 <= 65535 < 65543; 2048 - 255 * 8 = 8 >= 0 > -247;
# signed 2048 + 255 * 120 = 32648 <= 32767 < 32903; 2048 - 255 * 136 = -32632 >= -32768 > -32887
_pk16_1d_case("pk16-u-vmax-s0", *_pk_pair(5, 248, 0, 0, True), 12, 1)
_pk16_1d_case("pk16-u-vmin-s0", *_pk_pair(5, 100, 8, 0, False), 12, 1)
_pk16_1d_case("pk16-s-vmax-s0", *_pk_pair(5, 120, 9, 0, True), 12, 2)
_pk16_1d_case("pk16-s-vmin-s0", *_pk_pair(5, 50, 136, 0, False), 12, 2)
# s = 3, frac 12 (bias 256, shift 9): 256 + 255 * 255 = 65281 <= 65535 < 65536 (exactly 2^16); 256 - 255 = 1 >= 0 > -254;
# 256 + 255 * 127 = 32641 <= 32767 < 32896; 256 - 255 * 129 = -32639 >= -32768 > -32894
_pk16_1d_case("pk16-u-vmax-s3", *_pk_pair(3, 255, 0, 3, True), 12, 1, unit=8)
_pk16_1d_case("pk16-u-vmin-s3", *_pk_pair(5, 90, 1, 3, False), 12, 1, unit=8)
_pk16_1d_case("pk16-s-vmax-s3", *_pk_pair(5, 127, 5, 3, True), 12, 2, unit=8)
_pk16_1d_case("pk16-s-vmin-s3", *_pk_pair(5, 33, 129, 3, False), 12, 2, unit=8)
# f - s = 15 / 16 at frac 16: [2, 4, 2] has s = 1, [2, 5, 2] has s = 0 and its 16-bit shift by 16 would be a shift by 0
_pk16_1d_case("pk16-shift15-16", np.array([2, 4, 2]), np.array([2, 5, 2]), 16, 1,
              benign=np.array([0, 0, 1 << 12, 1 << 13, 1 << 12]))


def _hi8_case(cid, f, rej_bank, acc_bank=np.array([[0, 16, 0], [32, 16, 32], [48, 160, 48]])):
    """A bank whose filters are all unsigned with f - s == 8 stores V's high byte; the same bank
    with one tap of filter ``f`` moved by one unit of 2^s must not."""
    plan = _bank_plan(f)

    def narrow(x, side, stage):
        S = fo._mac_rows(np.asarray(x, np.int64), side.taps[f])
        return m_hi8(S, side.frac, plan(side)["s"])

    CASES.append(Case(cid, "plan_u8_pk16", "fir1d_reg.h:169-171", "bank", Side(acc_bank), Side(rej_bank),
                      lambda side: pk16_bank(side.taps, side.frac, side.acc)["hi8"], narrow, _pk_bounds(plan),
                      quantity=_pk_quantity(plan), unit=16, stages=(U8,), f=f))


# filter 0 turns signed ([0, 16, -16]); filter 1 goes to shift 7 ([32, 32, 32]: s = 5, its V's high byte is the output halved)
_hi8_case("pk16-hi8-signed", 0, np.array([[0, 16, -16], [32, 16, 32], [48, 160, 48]]))
_hi8_case("pk16-hi8-shift7", 1, np.array([[0, 16, 0], [32, 32, 32], [48, 160, 48]]))
SEAMS.append(dict(id="pk16-s-clamp", row="plan_u8_pk16", cite="fir1d_reg.h:152", kind="bank", dtype=np.uint8,
                  sides=[Side(np.array([[8, 24, 8], [4, 8, 4]]), 4), Side(np.array([[16, 48, 16], [4, 8, 4]]), 4),
                         Side(np.array([[32, 96, 32], [4, 8, 4]]), 4)], path=None, stages=(U8,),
                  value=lambda s: (common_shift(s.taps[0], 64), common_shift(s.taps[0], s.frac)), expect=[(3, 3), (4, 3), (5, 3)],
                  why="s = 3 is frac - 1: taps with four and five common zeros keep s = 3 and h >> s even"))

# -- row "launch_mfma_t": fir1d_mfma.hip:1023-1069 ---------------------------------------------
_MF = "fir1d_mfma.hip:1032-1033"
_p_fast_u8 = lambda side: nowrap(side.taps, side.frac, side.acc, 255)  # noqa: E731
_p_fast_i16 = lambda side: nowrap(side.taps, side.frac, side.acc, 32768)  # noqa: E731
for _L in (10, 33, 65, 66, 257):  # step kernel (2 and 3 k-steps), run kernel
    _nowrap_case(f"mfma-fast-u8-acc24-L{_L}", "launch_mfma_t", _MF, "rows", taps_1d(_L, 32888, sign=1 if _L % 2 else -1),
                 12, 24, 9, _p_fast_u8)
# int16, acc 32: 65535 * 32768 + 2048 < 2^31 <= 65536 * 32768 + 2048.  Negative taps: x = -32768 under every
# tap but the one of -1 (x = -32767 there) sums to 2^31 - 1, and the half carries it past 2^31: tight.
for _L in (10, 33, 65, 66, 483):  # step kernel, chunked long kernel (4 and 17 k-steps)
    _nowrap_case(f"mfma-fast-i16-acc32-neg-L{_L}", "launch_mfma_t", _MF, "rows", taps_1d(_L, 65535, first=1, sign=-1),
                 12, 32, None, _p_fast_i16, dtype=np.int16, xmax=(32767, 32768))
# Positive taps: x = -32768 sums to exactly -2^31 on the rejected side, which wraps nothing; the largest
# positive sum 32767 * sum|h| comes within the half of 2^31 from sum|h| = 65538 (2^31 - 2): conservative.
_nowrap_case("mfma-fast-i16-acc32-pos-L33", "launch_mfma_t", _MF, "rows", taps_1d(33, 65535, first=1), 12, 32, 3, _p_fast_i16,
             dtype=np.int16, xmax=(32767, 32768))
_nowrap_case("mfma-fast-i16-acc32-pos-L66", "launch_mfma_t", _MF, "rows", taps_1d(66, 65535, first=1), 12, 32, 3, _p_fast_i16,
             dtype=np.int16, xmax=(32767, 32768))


def _mfma_tap_case(cid, L, dtype):
    h = taps_1d(L, 3000, 2500)
    h[L // 3] = 32639
    CASES.append(Case(cid, "launch_mfma_t", "fir1d_mfma.hip:1059-1060", "rows", Side(h), Side(_bump(h, L // 3, 1)),
                      lambda side: mfma1d_taps_ok(side.taps),
                      lambda x, side, stage: fo.fir1d_rows(x, m_taps_byte_pair(side.taps), side.frac, side.acc, stage),
                      (lambda side: (255 * psum(side.taps), 255 * nsum(side.taps))) if dtype == np.uint8 else
                      (lambda side: (32767 * psum(side.taps) - 32768 * nsum(side.taps),
                                     -32768 * psum(side.taps) + 32767 * nsum(side.taps))), dtype=dtype))


_mfma_tap_case("mfma-tap-32639-u8-L17", 17, np.uint8)   # 32640: the LDS v_dot2 kernel takes it
_mfma_tap_case("mfma-tap-32639-i16-L17", 17, np.int16)
_mfma_tap_case("mfma-tap-32639-u8-L66", 66, np.uint8)
SEAMS.append(dict(id="mfma-frac22-23", row="launch_mfma_t", cite="fir1d_mfma.hip:1033", kind="rows", dtype=np.uint8,
                  sides=[Side(taps_1d(33, 30000, 20000), 22, 32), Side(taps_1d(33, 30000, 20000), 23, 32)], path=None,
                  stages=(U8, I32), value=lambda s: nowrap(s.taps, s.frac, s.acc), expect=[True, False],
                  why="255 * 50000 + 2^22 stays below 2^31: folding the half into the bias is exact at frac 23 too"))

# -- row "launch2d_reg": fir2d.hip:147-257 -----------------------------------------------------
_L2 = "fir2d.hip:155-157"
_p_nowrap2 = lambda side: nowrap(side.taps, side.frac, side.acc)  # noqa: E731
_nowrap_case("reg2d-nowrap-acc24-gen3x3", "launch2d_reg", _L2, "frame", taps_2d(3, 3, 32888), 12, 24, 9, _p_nowrap2, path="reg",
             frames2=True)
_nowrap_case("reg2d-nowrap-acc24-gen5x5", "launch2d_reg", _L2, "frame", taps_2d(5, 5, 32888, sign=-1), 12, 24, 9, _p_nowrap2,
             path="reg")
# 255 * 2055 + 128 = 524153 < 2^19 <= 255 * 2056 + 128 = 524408; the sum alone reaches 2^19 from 2057
_nowrap_case("reg2d-nowrap-acc20-gen3x3", "launch2d_reg", _L2, "frame", taps_2d(3, 3, 2055), 8, 20, 2, _p_nowrap2, path="reg")
# a rank-1 set (col [1, 1, 1] x row): one unit in the row factor is three units of sum|h|:
# 255 * 32886 + 2048 < 2^23 <= 255 * 32889 + 2048; the sum alone reaches 2^23 from 32898
_row_nw = taps_1d(3, 10962, first=3653)


def _sep_nowrap_case():
    a = outer([1, 1, 1], _row_nw)
    c = Case("reg2d-nowrap-acc24-sep3x3", "launch2d_reg", _L2, "frame", Side(a, 12, 24),
             Side(outer([1, 1, 1], _grow(_row_nw)), 12, 24), _p_nowrap2, None, _one_sided(255, 0),
             extra=Side(outer([1, 1, 1], _grow(_row_nw, 4)), 12, 24), unit=1, frames2=True)
    c.narrow = lambda x, side, stage: m_nowrap(c.sums(x, side), side.frac, stage)
    CASES.append(c)


_sep_nowrap_case()


def _sep_case(cid, col, row_accept, bits, cite):
    """The row factor's sum crosses the separable forms' limit by one unit in one row tap."""
    want = "sep16" if bits == 16 else "sep"
    row_reject = _grow(row_accept)
    CASES.append(Case(cid, "launch2d_reg", cite, "frame", Side(outer(col, row_accept)), Side(outer(col, row_reject)),
                      lambda side, want=want: sep_form(side.taps, side.frac, side.acc) in
                      (("sep16",) if want == "sep16" else ("sep16", "sep")),
                      lambda x, side, stage, bits=bits: np.stack([m_sep(f, side.taps, side.frac, side.acc, stage, bits) for f in x]),
                      _u8_bounds(), frames2=bits == 16))


# int16 row sums: 255 * 128 = 32640 <= 32767 < 255 * 129 = 32895.  col [1, 2, 1] keeps 255 sum|h| above
# 65535, so the packed-16 plan refuses and the u8 stage reaches the separable kernels too.
_sep_case("reg2d-sep16-3x3", [1, 2, 1], taps_1d(3, 128), 16, "fir2d.hip:176-179")
_sep_case("reg2d-sep16-5x5", [1, -2, 3, -2, 1], taps_1d(5, 128), 16, "fir2d.hip:176-179")
# 24-bit row sums: 255 * 32896 = 8388480 < 2^23 <= 255 * 32897
_sep_case("reg2d-sep24-3x3", [1, -1, 1], taps_1d(3, 32896), 24, "fir2d.hip:160-164")
_sep_case("reg2d-sep24-5x3", [1, 1, -1, 1, 1], taps_1d(3, 32896), 24, "fir2d.hip:160-164")



def _col16_case(cid, a, b):
    """The column factor crosses int16 (fir2d.hip:179): rank1_factor divides by a row tap of -1, so a tap of
    -32768 is a column tap of +32768, which the packed int16 column taps would hold as -32768."""
    def narrow(x, side, stage):
        return np.stack([m_sep(f, side.taps, side.frac, side.acc, stage, 16, col_bits=16) for f in x])

    CASES.append(Case(cid, "launch2d_reg", "fir2d.hip:179", "frame", Side(a), Side(b),
                      lambda side: sep_form(side.taps, side.frac, side.acc) == "sep16", narrow, _u8_bounds()))


# col 32767 / 32768: one tap of a kernel with one non-zero column; a whole row of taps of outer(col, [-1, -1, -1]),
# 3 and 5 rows.  255 * 3 row sums fit int16 easily; 255 sum|h| is far above 65535, so no packed-16 plan intervenes.
_c1 = np.array([[-1, 0, 0], [-32767, 0, 0], [0, 0, 0]])
_col16_case("reg2d-col16-one-tap-3x3", _c1, _bump(_c1, (1, 0), -1))
_col16_case("reg2d-col16-3x3", outer([1, 32767, 1], [-1, -1, -1]), outer([1, 32768, 1], [-1, -1, -1]))
_col16_case("reg2d-col16-5x3", outer([1, 0, 32767, -2, 1], [-1, -1, -1]), outer([1, 0, 32768, -2, 1], [-1, -1, -1]))

# -- row "plan_pk16": fir2d_reg.h:82-154 (u8 stage, FIR2D_PATH=reg; the rolled form: H * W < 2^31) ----
def _pk16_2d_case(cid, a, b, frac, want, unit=1, cite="fir2d_reg.h:135-146", frames2=False):
    def narrow(x, side, stage):
        sh = _frame_plan(side)["s"]
        S = np.stack([mac2d(f, side.taps) for f in x])
        return m_hi8(S, side.frac, sh) if want == "hi8" else m_pk16(S, side.frac, sh, want == 2)

    def pred(side):
        p = _frame_plan(side)
        if want == "hi8":
            return p["mode"] == 1 and side.frac - p["s"] == 8
        return p["mode"] == want

    CASES.append(Case(cid, "plan_pk16", cite, "frame", Side(a, frac), Side(b, frac), pred, narrow, _pk_bounds(_frame_plan),
                      quantity=_pk_quantity(_frame_plan), unit=unit, stages=(U8,), path="reg", frames2=frames2))


def _gen_pair(R, C, pos, neg, s, grow_pos):
    a = taps_2d(R, C, pos, neg, s)
    sel = np.argwhere(a > 0) if grow_pos else np.argwhere(a < 0)
    for i in [tuple(v) for v in sel[::-1]]:
        b = _bump(a, i, (1 << s) if grow_pos else -(1 << s))
        if common_shift(b, 64) == s and not is_rank1(b):
            return a, b
    raise AssertionError("no tap to grow")


for _R in (3, 5):  # general kernels: the same four ends as the 1-D bank, s = 0 and s = 3
    _g = f"gen{_R}x{_R}"
    _pk16_2d_case(f"pk16-2d-{_g}-u-vmax-s0", *_gen_pair(_R, _R, 248, 0, 0, True), 12, 1, frames2=_R == 3)
    _pk16_2d_case(f"pk16-2d-{_g}-u-vmin-s0", *_gen_pair(_R, _R, 100, 8, 0, False), 12, 1)
    _pk16_2d_case(f"pk16-2d-{_g}-s-vmax-s0", *_gen_pair(_R, _R, 120, 9, 0, True), 12, 2)
    _pk16_2d_case(f"pk16-2d-{_g}-s-vmin-s0", *_gen_pair(_R, _R, 50, 136, 0, False), 12, 2)
    _pk16_2d_case(f"pk16-2d-{_g}-u-vmax-s3", *_gen_pair(_R, _R, 255, 0, 3, True), 12, 1, unit=8)
    _pk16_2d_case(f"pk16-2d-{_g}-s-vmin-s3", *_gen_pair(_R, _R, 33, 129, 3, False), 12, 2, unit=8)
# hi8: f - s = 8 (s = 4): 128 + 255 * 256 = 65408 <= 65535 < 128 + 255 * 257 = 65663
_pk16_2d_case("pk16-2d-gen3x3-hi8-vmax", *_gen_pair(3, 3, 256, 0, 4, True), 12, "hi8", unit=16)
# f - s = 7 and 9: unsigned ends with the clamp in play: 64 + 255 * 256 = 65344 / 65599; 256 + 255 * 255 = 65281 / 65536
_pk16_2d_case("pk16-2d-gen3x3-u-vmax-s5", *_gen_pair(3, 3, 256, 0, 5, True), 12, 1, unit=32)
# rank-1 kernels (plan_pk16, fir2d_reg.h:82-118): col [1, 1, 1] x row, one unit in a row tap = R units of the sum:
# 2048 + 255 * 246 = 64778 <= 65535 < 2048 + 255 * 249 = 65543; 5x5: 2048 + 255 * 245 / 250
_RK = "fir2d_reg.h:93-110"
_r3, _r5 = taps_1d(3, 82), taps_1d(5, 49)
_pk16_2d_case("pk16-2d-sep3x3-u-vmax-s0", outer([1, 1, 1], _r3), outer([1, 1, 1], _grow(_r3)), 12, 1, cite=_RK, frames2=True)
_pk16_2d_case("pk16-2d-sep5x5-u-vmax-s0", outer([1] * 5, _r5), outer([1] * 5, _grow(_r5)), 12, 1, cite=_RK)
# signed: col [1, -1, 1]: vmax = 2048 + 255 * (2 P + N), vmin = 2048 - 255 * (2 N + P) with row sums P = 40, N = 40:
# vmax 32648 <= 32767 and one more unit of a positive row tap adds two: 2048 + 255 * 122 = 33158
_rs = taps_1d(3, 40, 40, first=19)
_pk16_2d_case("pk16-2d-sep3x3-s-vmax-s0", outer([1, -1, 1], _rs), outer([1, -1, 1], _grow(_rs)), 12, 2, cite=_RK)
# unsigned vmin, col of ones: 2048 - 255 * 3 * 2 = 518 >= 0 > 2048 - 255 * 3 * 3 = -247 (the signed form takes over);
# 5x5: 2048 - 255 * 5 * 1 = 773 >= 0 > 2048 - 255 * 5 * 2 = -502
_rn3, _rn5 = taps_1d(3, 30, 2, first=13), taps_1d(5, 20, 1)
_pk16_2d_case("pk16-2d-sep3x3-u-vmin-s0", outer([1, 1, 1], _rn3), outer([1, 1, 1], _grow_neg(_rn3)), 12, 1, cite=_RK)
_pk16_2d_case("pk16-2d-sep5x5-u-vmin-s0", outer([1] * 5, _rn5), outer([1] * 5, _grow_neg(_rn5)), 12, 1, cite=_RK)
# signed vmin, col [1, -1, 1] (products of two negative factor taps are positive): vmin = 2048 - 255 * (2 N + P),
# row sums P = 20, N = 58: 2048 - 255 * 136 = -32632 >= -32768 > 2048 - 255 * 137 = -32887
_rm3 = taps_1d(3, 20, 58, first=9)
_pk16_2d_case("pk16-2d-sep3x3-s-vmin-s0", outer([1, -1, 1], _rm3), outer([1, -1, 1], _grow(_rm3)), 12, 2, cite=_RK)
# 5x5, col [1, -1, 1, -1, 1]: vmin = 2048 - 255 * (3 N + 2 P), vmax = 2048 + 255 * (3 P + 2 N).  P = 8, N = 40:
# vmin -32632 / one more unit of a positive row tap: 2048 - 255 * 138 = -33142.  P = 30, N = 15: vmax 32648 / 33413
_rm5, _rx5 = taps_1d(5, 8, 40), taps_1d(5, 30, 15)
_alt5 = [1, -1, 1, -1, 1]
_pk16_2d_case("pk16-2d-sep5x5-s-vmin-s0", outer(_alt5, _rm5), outer(_alt5, _grow(_rm5)), 12, 2, cite=_RK)
_pk16_2d_case("pk16-2d-sep5x5-s-vmax-s0", outer(_alt5, _rx5), outer(_alt5, _grow(_rx5)), 12, 2, cite=_RK)
# rank1_factor divides the row factor by its gcd, so every common power of two sits in the column factor (zr = 0,
# sr = 0 always): col [4, 8, 4] x (row << 1) is planned as col [8, 16, 8] (zc = 3), s = sc = 3, bias 256, shift 9:
# 256 + 255 * 4 * 63 = 64516 <= 65535 < 256 + 255 * 4 * 64 = 65536
_r63 = taps_1d(3, 63, first=20)
_pk16_2d_case("pk16-2d-sep3x3-u-vmax-s3", outer([4, 8, 4], _r63 << 1), outer([4, 8, 4], _grow(_r63) << 1), 12, 1, cite=_RK)
# frac 2: s = min(zc, frac - 1) = 1 < zc = 2 (sc < zc): col >> 1 = [2, 2, 2] stays even; bias 1, shift 1:
# 1 + 255 * 6 * 42 = 64261 <= 65535 < 1 + 255 * 6 * 43 = 65791 (255 past 2^16: the wrapped V >> 1 is 127)
_r42 = taps_1d(3, 42, first=13)
_pk16_2d_case("pk16-2d-sep3x3-split-sc", outer([4, 4, 4], _r42), outer([4, 4, 4], _grow(_r42)), 2, 1, cite=_RK)
# hi8 for a rank-1 kernel: col [16, 16, 16] (s = 4), 128 + 255 * 3 * 85 = 65153 <= 65535 < 128 + 255 * 3 * 86 = 65918
_r85 = taps_1d(3, 85, first=28)
_pk16_2d_case("pk16-2d-sep3x3-hi8-vmax", outer([16, 16, 16], _r85), outer([16, 16, 16], _grow(_r85)), 12, "hi8", cite=_RK)

# -- row "plan_mfma2": fir2d_mfma.hip:355-401 (u8 stage) ----------------------------------------
def _mfma2_case(cid, a, b, frac, acc, pred, narrow, path, unit=1, extra=None, cite="fir2d_mfma.hip:370-375", frames2=False,
                bounds=None):
    CASES.append(Case(cid, "plan_mfma2", cite, "frame", Side(a, frac, acc), Side(b, frac, acc), pred, narrow,
                      bounds or _u8_bounds(), unit=unit, stages=(U8,), path=path, frames2=frames2,
                      extra=None if extra is None else Side(extra, frac, acc)))


def _m2_taps(x, side, stage, model):
    return np.stack([fo.fir2d_fixed(f, model(side.taps), side.frac, side.acc, stage) for f in x])


_p_np1 = lambda side: mfma2_plan(side.taps, side.frac, side.acc)["np"] == 1  # noqa: E731
_p_np = lambda side: mfma2_plan(side.taps, side.frac, side.acc)["np"] != 0  # noqa: E731
_p_m2fast = lambda side: mfma2_plan(side.taps, side.frac, side.acc)["fast"]  # noqa: E731
_n_byte = lambda x, side, stage: _m2_taps(x, side, stage, lambda h: m_taps_byte(h, mfma2_plan(h, side.frac, side.acc)["s"]))  # noqa: E731
_n_pair = lambda x, side, stage: _m2_taps(x, side, stage, m_taps_byte_pair)  # noqa: E731
_b3 = np.array([[1, -2, 3], [4, 127, -6], [7, 8, -9]])
_b5 = np.arange(-12, 13).reshape(5, 5) * 7 + 2
_b5[2, 2] = -128
for _path in (None, "mfma"):
    _t = "auto" if _path is None else "mfma"
    _mfma2_case(f"mfma2-np-127-3x3-{_t}", _b3, _bump(_b3, (1, 1), 1), 7, 32, _p_np1, _n_byte, _path, frames2=_path is None)
    _mfma2_case(f"mfma2-np--128-5x5-{_t}", _b5, _bump(_b5, (2, 2), -1), 10, 32, _p_np1, _n_byte, _path)
# the same with a common shift: taps >> 2 = 127 / 128, one unit = 4
_mfma2_case("mfma2-np-127-s2-3x3-auto", _b3 << 2, _bump(_b3 << 2, (1, 1), 4), 9, 32, _p_np1, _n_byte, None, unit=4)
_w3 = np.array([[-30000, 29001, 1], [32639, -32768, 77], [5, -20001, 31001]])
_mfma2_case("mfma2-tap-32639-3x3-auto", _w3, _bump(_w3, (1, 0), 1), 12, 32, _p_np, _n_pair, None)
_mfma2_case("mfma2-tap-32639-3x3-mfma", _w3, _bump(_w3, (1, 0), 1), 12, 32, _p_np, _n_pair, "mfma")


def _n_m2fast(x, side, stage):
    return m_mfma2_fast(np.stack([mac2d(f, side.taps) for f in x]), side.frac)


# frac 12: 255 * 526336 = 2^27 - 2048 exactly, so (255 * 526336 + 2048) << 4 = 2^31 and one unit less gives
# 2^31 - 4080: tight
_f5 = taps_2d(5, 5, 526335, hmax=32639)
_mfma2_case("mfma2-fast-f12-5x5-auto", _f5, _grow(_f5), 12, 32, _p_m2fast, _n_m2fast, None, cite="fir2d_mfma.hip:390-391",
            bounds=_one_sided(255, 0), frames2=True)
# negative taps: the bound is symmetric but int32 is not, and the half helps: (-255 * sum|h| + 2048) << 4 stays
# above -2^31 up to sum|h| = 526352: conservative by 17 units
_mfma2_case("mfma2-fast-f12-5x5-neg-mfma", -_f5, _grow(-_f5), 12, 32, _p_m2fast, _n_m2fast, "mfma", cite="fir2d_mfma.hip:390-391",
            bounds=_one_sided(255, 0), extra=_grow(-_f5, 18))
# acc 24 (the nowrap half of `fast`): as launch_reg's, conservative by the rounding half
_g3 = taps_2d(3, 3, 32888)
_mfma2_case("mfma2-fast-acc24-3x3-auto", _g3, _grow(_g3), 12, 24, _p_m2fast,
            lambda x, side, stage: m_nowrap(np.stack([mac2d(f, side.taps) for f in x]), side.frac, stage), None,
            extra=_grow(_g3, 9), cite="fir2d_mfma.hip:390-391", bounds=_one_sided(255, 0))
SEAMS.append(dict(id="mfma2-frac16-17", row="plan_mfma2", cite="fir2d_mfma.hip:391", kind="frame", dtype=np.uint8,
                  sides=[Side(taps_2d(3, 3, 9000, 5000), 16, 32), Side(taps_2d(3, 3, 9000, 5000), 17, 32)], path=None,
                  stages=(U8,), value=lambda s: mfma2_plan(s.taps, s.frac, s.acc)["fast"], expect=[True, False],
                  why="frac 17 would need a right shift where the fast form shifts left: a form limit, not a range"))
SEAMS.append(dict(id="mfma2-s-clamp", row="plan_mfma2", cite="fir2d_mfma.hip:369", kind="frame", dtype=np.uint8,
                  sides=[Side(_b3 << 3, 4, 32), Side(_b3 << 4, 4, 32), Side(_b3 << 5, 4, 32)], path="mfma", stages=(U8,),
                  value=lambda s: (common_shift(s.taps, 64), mfma2_plan(s.taps, s.frac, s.acc)["s"], mfma2_plan(s.taps, s.frac, s.acc)["np"]),
                  expect=[(3, 3, 1), (4, 3, 2), (5, 3, 2)],
                  why="s = 3 is frac - 1: taps with more common zeros keep s = 3, and their >> s may leave a byte"))


# -- row "needs_wide": fir1d.hip:159-165, int16 samples, acc_bits = 64 ---------------------------
def wide_case():
    """2^17 taps of -2^31 (the last one -2^31 + 1 on the accepted side): sum|h| = 2^48 - 1 / 2^48,
    and x = -32768 under every tap sums to 2^63 - 32768 / exactly 2^63 (in one shard of 1024
    outputs with its halos).  At acc_bits = 64 the reference wraps 2^63 to -2^63 itself, so the
    proof is conservative there; from acc_bits = 65 a 64-bit sum is wrong on the rejected side.
    Returns (accept taps, reject taps)."""
    h = np.full(1 << 17, -(1 << 31), np.int64)
    return _bump(h, -1, 1), h


# ---- the narrow form of each case, as a launch shows it -----------------------------------------
_REG1D = ("fir1d_reg_kernel", "fir1d_reg_batch_kernel")
_REG2D = ("fir2d_reg_kernel", "fir2d_pk16_strip_kernel")


def _f_u8dot2(l):  # byte-pair v_dot2: no accumulator can wrap, int16 taps
    return l.kernel in _REG1D and "kU8Dot2" in l.flags


def _f_pk16_bank(l):  # the bank kernel with packed-16 filters (which filters: TapsN::pkmode, run time)
    return l.kernel in _REG1D and "kU8Pk16" in l.flags


def _f_mfma_fast(l):  # the matrix-core kernels' FAST form (template argument; the run kernel: its mode)
    return ((l.kernel == "fir1d_mfma_step_kernel" and l.targs[4] == "true")
            or (l.kernel == "fir1d_mfma_long_kernel" and l.targs[3] == "true")
            or (l.kernel == "fir1d_mfma_run_kernel" and l.note.get("mode") == "fast"))


def _f_mfma(l):
    return l.kernel.startswith("fir1d_mfma_")


def _f_nowrap2d(l):  # the strip kernel is taken only under nowrap (fir2d.hip:188)
    return l.kernel == "fir2d_pk16_strip_kernel" or (l.kernel == "fir2d_reg_kernel" and "nowrap" in l.flags)


def _f_sep16(l):
    return l.kernel == "fir2d_reg_kernel" and "sep16" in l.flags


def _f_sep(l):
    return l.kernel == "fir2d_pk16_strip_kernel" or (l.kernel == "fir2d_reg_kernel" and "sep" in l.flags)


def _f_pk_unsigned(l):
    return l.kernel in _REG2D and "pk16" in l.flags and "pksigned" not in l.flags


def _f_pk_signed(l):
    return l.kernel in _REG2D and "pksigned" in l.flags


def _f_pk_any(l):
    return l.kernel in _REG2D and "pk16" in l.flags


def _f_pk_hi8(l):
    return l.kernel in _REG2D and "pkhi8" in l.flags


def _f_m2(l):
    return l.kernel == "fir2d_mfma_kernel"


def _f_m2_np1(l):
    return l.kernel == "fir2d_mfma_kernel" and l.targs[1] == "1"


def _f_m2_fast(l):
    return l.kernel == "fir2d_mfma_kernel" and l.targs[2] == "true"


# id prefix -> (form, runtime); the first match holds
_FORMS = [
    ("reg-nowrap", _f_u8dot2, False), ("reg-taps16", _f_u8dot2, False),
    ("noclamp-", _f_u8dot2, True),      # plan_u8_noclamp sets TapsN's clamp bound, read at run time
    ("pk16-2d-gen3x3-hi8", _f_pk_hi8, False), ("pk16-2d-sep3x3-hi8", _f_pk_hi8, False),
    ("pk16-2d-gen3x3-u", _f_pk_unsigned, False), ("pk16-2d-gen5x5-u", _f_pk_unsigned, False),
    ("pk16-2d-sep3x3-u", _f_pk_unsigned, False), ("pk16-2d-sep5x5-u", _f_pk_unsigned, False),
    ("pk16-2d-gen3x3-s", _f_pk_signed, False), ("pk16-2d-gen5x5-s", _f_pk_signed, False),
    ("pk16-2d-sep3x3-s-", _f_pk_signed, False), ("pk16-2d-sep5x5-s-", _f_pk_signed, False),
    ("pk16-2d-sep3x3-split-sc", _f_pk_any, False),
    ("pk16-", _f_pk16_bank, True),      # plan_u8_pk16 sets each filter's TapsN::pkmode, read at run time
    ("mfma-fast", _f_mfma_fast, False), ("mfma-tap-32639", _f_mfma, False),
    ("reg2d-nowrap", _f_nowrap2d, False), ("reg2d-sep16", _f_sep16, False), ("reg2d-sep24", _f_sep, False),
    ("reg2d-col16", _f_sep16, False),
    ("mfma2-np", _f_m2_np1, False), ("mfma2-tap-32639", _f_m2, False), ("mfma2-fast", _f_m2_fast, False),
]
for _c in CASES:
    for _prefix, _form, _runtime in _FORMS:
        if _c.id.startswith(_prefix):
            _c.form, _c.runtime = _form, _runtime
            break
    assert _c.form is not None, _c.id

# the seams: the form and on which sides a launch shows it
for _sid, _form, _launched in (("reg-frac22-23", _f_u8dot2, [True, False]), ("pk16-s-clamp", _f_pk16_bank, [True, True, True]),
                               ("mfma-frac22-23", _f_mfma_fast, [True, False]), ("mfma2-frac16-17", _f_m2_fast, [True, False]),
                               ("mfma2-s-clamp", _f_m2_np1, [True, False, False])):
    _s = next(s for s in SEAMS if s["id"] == _sid)
    _s["form"], _s["launched"] = _form, _launched
assert all("form" in s and len(s["launched"]) == len(s["sides"]) for s in SEAMS)

CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)
ROWS = ["launch_reg", "plan_u8_noclamp", "plan_u8_pk16", "launch_mfma_t", "launch2d_reg", "plan_pk16", "plan_mfma2"]
