"""Reference, predicted dispatch and shapes of the streaming U/D resampling complex-tap FIR
(include/fir_crstream.h) -- a test helper, not a test module.

``want_block``: what fir_cplx_rstream_block must give, from the header's identity 2.  With
H = (taps - 1) // U, c0 = taps // 2 and Z = one zero frame ++ hist ++ x (1 + H + width frames), the
causal sum s[j] is frame j + (H + 1) * U - c0 of the one-shot interpolator over Z, whose reference is
tests/cinterp_cases.py's ``want`` (two real filters of the committed C oracle on the zero-stuffed
signal); so y is frames ``[phase + (H + 1) * U - c0 :: D][: out_width]`` of that array, hist_out the
last H frames of Z and next_phase = phase + out_width * D - width * U.  ``want_block_loop`` is the
header's causal formula itself in Python ints, over the kept frames only and without Z: the only
reference once a sum can pass 2^63; tests/test_crstream_cases.py holds the first against the second.

``predicted_route``: the FIR kernel a call takes, written from the header's "Routes" section, never by
asking the library.

The fast kernel's constants are the one-shot resampler's (tests/cresample_cases.py: a workgroup owns
P = periods(D) periods of D input and U output frames, in tiles of T = tile(U, D) periods); its plan
is causal (``phases``), and ``window_start`` is S, the first frame of a period's lowest window.
"""
from __future__ import annotations

import numpy as np

import cinterp_cases
import cresample_cases as cr

OUT_U8_SAT, OUT_I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)  # FIR_CRSTREAM_*
BUCKETS = cr.BUCKETS
PASS, W, MAX_UD, MAX_TAPS, MAX_PER_PHASE, ROW_UNIT = cr.PASS, cr.W, cr.MAX_UD, cr.MAX_TAPS, cr.MAX_PER_PHASE, cr.ROW_UNIT
periods, tile, frames, taps, sum_can_pass_2_63 = cr.periods, cr.tile, cr.frames, cr.taps, cr.sum_can_pass_2_63


def hist_frames(L: int, U: int) -> int:
    return (L - 1) // U


def out_width(width: int, U: int, D: int, phase: int) -> int:
    return -(-(width * U - phase) // D) if width * U > phase else 0


def next_phase(width: int, U: int, D: int, phase: int) -> int:
    return phase + out_width(width, U, D, phase) * D - width * U


def _taps_of(hq) -> int:
    return np.asarray(hq).reshape(-1, 2).shape[0]


def want_block(x, hist, hq, U: int, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32):
    """(y, hist_out, next_phase) over the committed C oracle (identity 2)."""
    x = np.asarray(x, dtype=np.int16)
    lead, width = x.shape[:-1], x.shape[-1] // 2
    L = _taps_of(hq)
    H, c0 = hist_frames(L, U), L // 2
    if hist is None:
        hist = np.zeros(lead + (2 * H,), np.int16)
    assert hist.shape == lead + (2 * H,) and hist.dtype == np.int16
    z = np.concatenate([np.zeros(lead + (2,), np.int16), hist, x], axis=-1)
    ow = out_width(width, U, D, phase)
    dtype = np.uint8 if stage == OUT_U8_SAT else np.int32
    if ow:
        full = cinterp_cases.want(z, hq, U, frac, acc, stage)
        first = phase + (H + 1) * U - c0
        assert first >= 0 and first + (ow - 1) * D < (1 + H + width) * U
        fr = full.reshape(lead + ((1 + H + width) * U, 2))[..., first::D, :][..., :ow, :]
        y = np.ascontiguousarray(fr).reshape(lead + (2 * ow,)).astype(dtype, copy=False)
    else:
        y = np.zeros(lead + (0,), dtype)
    hist_out = np.ascontiguousarray(z[..., z.shape[-1] - 2 * H:])
    return y, hist_out, next_phase(width, U, D, phase)


def want_block_loop(x, hist, hq, U: int, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32):
    """The header's causal sums as Python ints (NumPy object arrays), over the kept frames only: kept
    frame m is intermediate frame j = phase + m * D, e = j mod U, i = j div U, and sums the taps
    e + U t over the frames X[i - t], X = hist ++ x."""
    x = np.asarray(x, dtype=np.int16)
    lead, width = x.shape[:-1], x.shape[-1] // 2
    h = np.asarray(hq, dtype=object).reshape(-1, 2)
    L = h.shape[0]
    H = hist_frames(L, U)
    if hist is None:
        hist = np.zeros(lead + (2 * H,), np.int16)
    assert hist.shape == lead + (2 * H,) and hist.dtype == np.int16
    z = np.concatenate([hist, x], axis=-1)
    z2 = z.reshape(int(np.prod(lead, dtype=np.int64)), z.shape[-1])
    zo = z2.astype(object).reshape(z2.shape[0], H + width, 2)
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)

    def finish(v: int) -> int:  # cplx_ref.cplx_loop's
        v &= mask
        if v & sign:
            v -= 1 << acc
        v = (v + bias) >> frac
        if stage == OUT_U8_SAT:
            return 0 if v < 0 else (255 if v > 255 else v)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)

    ow = out_width(width, U, D, phase)
    y = np.zeros((z2.shape[0], 2 * ow), np.uint8 if stage == OUT_U8_SAT else np.int32)
    for m in range(ow):
        i, e = divmod(phase + m * D, U)
        sub = h[e::U]  # tap e + U t, t = 0 .. n - 1
        n = sub.shape[0]
        if not n:
            continue
        assert n - 1 <= H and i < width
        for r in range(z2.shape[0]):
            win = zo[r, H + i - (n - 1):H + i + 1][::-1]  # frames X[i - t]
            wr, wi = win[:, 0], win[:, 1]
            y[r, 2 * m] = finish(int(np.dot(sub[:, 0], wr) - np.dot(sub[:, 1], wi)))
            y[r, 2 * m + 1] = finish(int(np.dot(sub[:, 0], wi) + np.dot(sub[:, 1], wr)))
    hist_out = np.ascontiguousarray(z[..., z.shape[-1] - 2 * H:])
    return y.reshape(lead + (2 * ow,)), hist_out, next_phase(width, U, D, phase)


def run_split(block, x, hist, hq, U, D, phase, widths, *a):
    """``block`` (want_block's signature and result) over consecutive blocks of the given widths with
    the history and the phase carried: (the outputs concatenated, the final history, the final phase)."""
    assert sum(widths) == x.shape[-1] // 2
    ys, at = [], 0
    for w in widths:
        y, hist, phase = block(x[..., 2 * at:2 * (at + w)], hist, hq, U, D, phase, *a)
        ys.append(y)
        at += w
    if hist is None:  # no block at all
        hist = np.zeros(x.shape[:-1] + (2 * hist_frames(_taps_of(hq), U),), np.int16)
    return np.concatenate(ys, axis=-1) if ys else None, hist, phase


# ---- the fast kernel's causal plan (the header's FIR_CRSTREAM_FAST paragraph) ------------------------
def phases(L: int, U: int, D: int, phase: int) -> list:
    """(p_q, c_q, n_q) for q = 0 .. U - 1, from a_q = phase + q * D."""
    out = []
    for q in range(U):
        a = phase + q * D
        p, c = a % U, a // U
        out.append((p, c, -(-(L - p) // U) if p < L else 0))
    return out


def bucket(L: int, U: int, D: int, phase: int) -> int:
    """The smallest bucket that holds the longest sub-filter (1 when every phase is empty)."""
    need = max(n for _, _, n in phases(L, U, D, phase))
    return min(b for b in BUCKETS if b >= need)


def window_start(L: int, U: int, D: int, phase: int) -> int:
    """S: the lowest first frame c_q - n_q + 1 of a period's windows (0 when every phase is empty)."""
    return min((c - n + 1 for _, c, n in phases(L, U, D, phase) if n), default=0)


def predicted_route(x_addr: int, hist_in_addr: int, y_addr: int, hist_out_addr: int, rows: int, width: int, hq, U: int,
                    D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> tuple:
    """(route, tap bucket) from the header's "Routes" section; an address of 0 is NULL; y may sit at
    any element address."""
    ow = out_width(width, U, D, phase)
    if rows == 0 or ow == 0:
        return NONE, 0
    parts = np.asarray(hq).astype(np.int64).reshape(-1)
    L = len(parts) // 2
    dot2 = int(np.abs(parts).max()) <= 32767 and acc <= 32 and frac <= 31
    hist4 = hist_frames(L, U) == 0 or (hist_in_addr % 4 == 0 and hist_out_addr % 4 == 0)  # where they are given and H > 0
    if (dot2 and hist4 and 2 <= U <= MAX_UD and 2 <= D <= MAX_UD and L <= MAX_TAPS and -(-L // U) <= MAX_PER_PHASE
            and stage == OUT_I32 and x_addr % 16 == 0 and (rows == 1 or width % ROW_UNIT == 0) and width < 1 << 40
            and rows * -(-ow // (periods(D) * U)) < 1 << 31):
        return FAST, bucket(L, U, D, phase)
    if dot2 and hist4 and x_addr % 4 == 0:
        return GENERIC32, 0
    if acc >= 64 and sum_can_pass_2_63(hq):
        return GENERIC128, 0
    return GENERIC64, 0


# ---- shapes and inputs -------------------------------------------------------------------------------
def edge_widths(U: int, D: int) -> list:
    """Input widths around the output edges: the width of one output frame, and for a tile's (T U) and a
    workgroup's (P U) last output frame e the smallest widths that give at least e - 1, e and e + 1
    output frames at phase 0 (so the block's last frame lies just below, at or just past the edge)."""
    out = {1}
    for e in (tile(U, D) * U, periods(D) * U):
        out |= {-(-((o - 1) * D + 1) // U) for o in (e - 1, e, e + 1)}
    return sorted(out)


def hostile_history(rng, rows: int, H: int) -> np.ndarray:
    """A random history with frames of +-32767 / -32768 among it."""
    h = rng.integers(-32768, 32768, (rows, 2 * H), dtype=np.int16)
    ends = np.array([32767, -32768, -32767], np.int16)
    mask = rng.integers(0, 3, h.shape) == 0
    h[mask] = ends[rng.integers(0, 3, int(mask.sum()))]
    return h


def random_split(rng, n: int, hi: int) -> list:
    """Widths in [0, hi] that sum to n."""
    out = []
    while n:
        w = min(int(rng.integers(0, hi + 1)), n)
        out.append(w)
        n -= w
    return out
