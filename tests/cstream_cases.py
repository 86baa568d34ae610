"""Reference, predicted dispatch and shapes of the streaming decimating complex-tap FIR
(include/fir_cstream.h) -- a test helper, not a test module.

``want_block``: what fir_cplx_stream_block must give, from the header's identity 2.  With H = taps - 1,
c = taps // 2 and Z = hist ++ x (H + width frames), the causal sum s[n] is frame n + H - c of the
full-rate complex-tap FIR over Z, whose reference is tests/cplx_ref.py's ``want`` (two real filters of
the committed C oracle); so y is frames ``[phase + H - c :: D][: out_width]`` of that array, hist_out
the last H frames of Z and next_phase = phase + out_width * D - width.  ``want_block_loop`` is the same
over ``cplx_loop`` (plain Python ints), the only reference once a sum can pass 2^63;
tests/test_cstream_cases.py holds the first against the second.

``predicted_route``: the FIR kernel a call takes, written from the header's "Routes" section, never by
asking the library.

The fast kernel's constants are the decimator's (tests/cdecim_cases.py: T = 512 output frames per tile,
G = max(1, 16 / D) tiles per workgroup).
"""
from __future__ import annotations

import numpy as np

import cdecim_cases as dc
import cplx_ref

OUT_U8_SAT, OUT_I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)  # FIR_CSTREAM_*
BUCKETS = dc.BUCKETS
T, W, MAX_D, MAX_TAPS, ROW_UNIT = dc.T, dc.W, dc.MAX_D, dc.MAX_TAPS, dc.ROW_UNIT
tiles_per_group, out_width, frames, taps = dc.tiles_per_group, dc.out_width, dc.frames, dc.taps


def next_phase(width: int, D: int, phase: int) -> int:
    return phase + out_width(width, D, phase) * D - width


def _block(full_rate, x, hist, hq, D, phase, frac, acc, stage):
    x = np.asarray(x, dtype=np.int16)
    lead, width = x.shape[:-1], x.shape[-1] // 2
    L = np.asarray(hq).reshape(-1, 2).shape[0]
    H, c = L - 1, L // 2
    if hist is None:
        hist = np.zeros(lead + (2 * H,), np.int16)
    assert hist.shape == lead + (2 * H,) and hist.dtype == np.int16
    z = np.concatenate([hist, x], axis=-1)
    ow = out_width(width, D, phase)
    dtype = np.uint8 if stage == OUT_U8_SAT else np.int32
    if ow:
        full = full_rate(z, hq, frac, acc, stage)
        fr = full.reshape(lead + (H + width, 2))[..., phase + H - c::D, :][..., :ow, :]
        y = np.ascontiguousarray(fr).reshape(lead + (2 * ow,)).astype(dtype, copy=False)
    else:
        y = np.zeros(lead + (0,), dtype)
    hist_out = np.ascontiguousarray(z[..., z.shape[-1] - 2 * H:])
    return y, hist_out, next_phase(width, D, phase)


def want_block(x, hist, hq, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32):
    """(y, hist_out, next_phase) over the committed C oracle."""
    return _block(cplx_ref.want, x, hist, hq, D, phase, frac, acc, stage)


def want_block_loop(x, hist, hq, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32):
    """The same over the Python-int loop (small inputs only)."""
    return _block(cplx_ref.cplx_loop, x, hist, hq, D, phase, frac, acc, stage)


def want_block_kept(x, hist, hq, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32):
    """The header's causal sums as Python ints (NumPy object arrays), over the KEPT frames only: the
    reference when the taps are too many for a full-rate loop over hist ++ x (the 128-bit route needs
    2^16 taps and more).  tests/test_cstream_cases.py holds it against want_block_loop."""
    x = np.asarray(x, dtype=np.int16)
    rows, width = x.shape[0], x.shape[1] // 2
    h = np.asarray(hq, dtype=object).reshape(-1, 2)[::-1]  # window order: frame n - H + p meets tap L - 1 - p
    L = h.shape[0]
    H = L - 1
    if hist is None:
        hist = np.zeros((rows, 2 * H), np.int16)
    z = np.concatenate([hist, x], axis=1)
    zo = z.astype(object).reshape(rows, H + width, 2)
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)

    def finish(v: int) -> int:  # cplx_ref.cplx_loop's
        v &= mask
        if v & sign:
            v -= 1 << acc
        v = (v + bias) >> frac
        if stage == OUT_U8_SAT:
            return 0 if v < 0 else (255 if v > 255 else v)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)

    kept = range(phase, width, D)
    y = np.zeros((rows, 2 * len(kept)), np.uint8 if stage == OUT_U8_SAT else np.int32)
    for r in range(rows):
        for m, n in enumerate(kept):
            wr, wi = zo[r, n:n + L, 0], zo[r, n:n + L, 1]
            y[r, 2 * m] = finish(int(np.dot(h[:, 0], wr) - np.dot(h[:, 1], wi)))
            y[r, 2 * m + 1] = finish(int(np.dot(h[:, 0], wi) + np.dot(h[:, 1], wr)))
    return y, np.ascontiguousarray(z[:, z.shape[1] - 2 * H:]), next_phase(width, D, phase)


def run_split(block, x, hist, hq, D, phase, widths, *a):
    """``block`` (want_block's signature and result) over consecutive blocks of the given widths with
    the history and the phase carried: (the outputs concatenated, the final history, the final phase)."""
    assert sum(widths) == x.shape[-1] // 2
    ys, at = [], 0
    for w in widths:
        y, hist, phase = block(x[..., 2 * at:2 * (at + w)], hist, hq, D, phase, *a)
        ys.append(y)
        at += w
    if hist is None:  # no block at all
        hist = np.zeros(x.shape[:-1] + (2 * (np.asarray(hq).reshape(-1, 2).shape[0] - 1),), np.int16)
    return np.concatenate(ys, axis=-1) if ys else None, hist, phase


def predicted_route(x_addr: int, hist_in_addr: int, y_addr: int, hist_out_addr: int, rows: int, width: int, hq, D: int,
                    phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> tuple:
    """(route, tap bucket) from the header's "Routes" section; an address of 0 is NULL; y may sit at
    any element address."""
    ow = out_width(width, D, phase)
    if rows == 0 or ow == 0:
        return NONE, 0
    parts = np.asarray(hq).astype(np.int64).reshape(-1)
    L = len(parts) // 2
    dot2 = int(np.abs(parts).max()) <= 32767 and acc <= 32 and frac <= 31
    hist4 = L == 1 or (hist_in_addr % 4 == 0 and hist_out_addr % 4 == 0)  # where they are given and H > 0
    tiles = -(-ow // T)
    if (dot2 and hist4 and 2 <= D <= MAX_D and L <= MAX_TAPS and stage == OUT_I32 and x_addr % 16 == 0
            and (rows == 1 or width % ROW_UNIT == 0) and width < 1 << 40 and rows * tiles < 1 << 31):
        return FAST, min(b for b in BUCKETS if b >= L)
    if dot2 and hist4 and x_addr % 4 == 0:
        return GENERIC32, 0
    if acc >= 64 and dc.sum_can_pass_2_63(hq):
        return GENERIC128, 0
    return GENERIC64, 0


# ---- inputs ------------------------------------------------------------------------------------------
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
