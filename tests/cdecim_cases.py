"""Reference, predicted dispatch and shapes of the decimating complex-tap FIR (include/fir_cdecim.h)
-- a test helper, not a test module.

``want``: what fir_cplx_decim_rows must give.  The contract is ``y[r, m, :] = y_full[r, m * D + phase, :]``
with y_full the full-rate complex-tap FIR, whose reference is tests/cplx_ref.py's ``want`` (two real
filters of the committed C oracle); so this is that array viewed as frames and sliced
``[..., phase::D, :]``.  ``want_loop`` is the same slice of ``cplx_loop`` (plain Python ints), the only
reference once a sum can pass 2^63; tests/test_cdecim_cases.py holds the first against the second.

``predicted_route``: the kernel a call takes, written from the conditions the header documents, never
by asking the library.

The shape lists are in terms of the fast kernel's constants (csrc_cdecim/fir1d_cplx_decim.hip):
T = 512 output frames per tile, a lane owns outputs u and u + 256 of a tile (so a lane's first output
ends at 1 and a wave's first run of outputs at W = 64), G = max(1, 16 / D) tiles per workgroup.
"""
from __future__ import annotations

import numpy as np

import cplx_ref

OUT_U8_SAT, OUT_I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)  # FIR_CDECIM_*
BUCKETS = (2, 4, 6, 8, 12, 16, 24, 32, 48, 64)
T, W, MAX_D, MAX_TAPS, ROW_UNIT = 512, 64, 16, 64, 4     # kTileT, kWave, kTileMaxD, kTileMaxTaps, kChunk


def tiles_per_group(D: int) -> int:
    return max(1, MAX_D // D)


def out_width(width: int, D: int, phase: int) -> int:
    return len(range(phase, width, D))


def sliced(full: np.ndarray, D: int, phase: int) -> np.ndarray:
    frames = full.reshape(full.shape[:-1] + (full.shape[-1] // 2, 2))[..., phase::D, :]
    return np.ascontiguousarray(frames).reshape(full.shape[:-1] + (-1,))


def want(x, hq, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    return sliced(cplx_ref.want(x, hq, frac, acc, stage), D, phase)


def want_loop(x, hq, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    return sliced(cplx_ref.cplx_loop(x, hq, frac, acc, stage), D, phase)


def _parts(hq) -> np.ndarray:
    """The 2 * taps tap parts as a flat int64 array (they fit in int32)."""
    return np.asarray(hq).astype(np.int64).reshape(-1)


def sum_can_pass_2_63(hq) -> bool:
    """The restated needs_wide bound: sum_k (|hr[k]| + |hi[k]|) * 32768 could reach 2^63."""
    return int(np.abs(_parts(hq)).sum()) * 32768 >= 1 << 63  # the int64 sum is at most 2^31 * 2^31


def predicted_route(x_addr: int, y_addr: int, rows: int, width: int, hq, D: int, phase: int = 0, frac: int = 12,
                    acc: int = 32, stage: int = OUT_I32) -> tuple:
    """(route, tap bucket) from the header's "Dispatch" section; y may sit at any element address."""
    ow = out_width(width, D, phase)
    if rows == 0 or ow == 0:
        return NONE, 0
    parts = _parts(hq)
    L = len(parts) // 2
    dot2 = int(np.abs(parts).max()) <= 32767 and acc <= 32 and frac <= 31
    tiles = -(-ow // T)
    if (dot2 and 2 <= D <= MAX_D and L <= MAX_TAPS and stage == OUT_I32 and x_addr % 16 == 0
            and (rows == 1 or width % ROW_UNIT == 0) and width < 1 << 40 and rows * tiles < 1 << 31):
        return FAST, min(b for b in BUCKETS if b >= L)
    if dot2 and x_addr % 4 == 0:
        return GENERIC32, 0
    if acc >= 64 and sum_can_pass_2_63(hq):
        return GENERIC128, 0
    return GENERIC64, 0


# ---- shapes ----------------------------------------------------------------------------------------
def edge_out_widths(D: int) -> list:
    """Output widths one below, at and one past: one lane's outputs (1 and 257: lane 0's two), a
    wave's (W), a tile (T), a workgroup (G T) and two workgroups (2 G T)."""
    G = tiles_per_group(D)
    marks = (1, W, T // 2 + 1, T, G * T, 2 * G * T)
    return sorted({m + d for m in marks for d in (-1, 0, 1) if m + d >= 1})


def width_for(ow: int, D: int, phase: int, slack: int = 0) -> int:
    """A row width whose out_width is ow: the smallest one plus slack frames (slack < D keeps ow)."""
    assert 0 <= slack < D
    w = (ow - 1) * D + phase + 1 + slack
    assert out_width(w, D, phase) == ow
    return w


def multi_row_shapes(D: int) -> list:
    """(rows, width): rows of a multiple of 4 frames, down to rows far narrower than a 64-tap window,
    up to rows of one workgroup's input and one chunk more."""
    G = tiles_per_group(D)
    return [(3, 4), (5, 8), (300, 4), (7, 12), (5, 1028), (3, G * T * D), (2, G * T * D + 4), (9, 252)]


def frames(rng, rows: int, width: int) -> np.ndarray:
    return rng.integers(-32768, 32768, (rows, 2 * width), dtype=np.int16)


def taps(rng, L: int, lo: int = -3000, hi: int = 3001) -> np.ndarray:
    h = rng.integers(lo, hi, (L, 2))
    h[L // 2, 1] = 77  # never all real
    return h


# ---- random cases ----------------------------------------------------------------------------------
# Drawn with the helpers of tests/rate_property_cases.py (rates, tap values, bit widths, samples).
# `why` names what keeps a case off the fast kernel ("" : nothing), so that about half the cases
# take it and every reason of the header's "Dispatch" section is drawn on its own.
WHY = ("", "", "", "", "", "", "rate", "taps", "value", "bits", "stage", "shape", "align")
PROPERTY_MAX_WIDTH, PROPERTY_MAX_TAPS, PROPERTY_MAX_FRAMES = 5000, 70, 20000


def property_case():
    import math

    from hypothesis import strategies as st

    import rate_property_cases as rc

    @st.composite
    def case(draw):
        why = WHY[(draw(rc._SEED) * 2654435761 % 2**32 * len(WHY)) >> 32]  # hashed, as rc._route_and_reasons
        D = draw(st.one_of(st.just(1), rc._ABOVE_RATE) if why == "rate" else rc._IN_RATE)
        phase = draw(st.one_of(st.just(0), st.just(D - 1), st.integers(0, D - 1)))
        near = sorted({min(MAX_TAPS, max(1, b + d)) for b in BUCKETS for d in (-1, 0, 1)})
        L = draw(st.integers(MAX_TAPS + 1, PROPERTY_MAX_TAPS) if why == "taps" else
                 st.one_of(st.integers(1, 9), st.integers(1, MAX_TAPS), st.sampled_from(near)))
        kinds = ["q412", "q412", "small", "int16", "ends"] + (["mad24", "wide"] if why == "value" else [])
        h = rc._zero_some(draw, rc._tap_values(draw, 2 * L, kinds, -32767), 4).reshape(L, 2)
        if draw(st.integers(0, 7)) == 0:
            h[:, draw(st.integers(0, 1))] = 0  # purely real or purely imaginary taps
        if why == "value":  # whatever the kind drew, one part is outside [-32767, 32767]
            h[draw(st.integers(0, L - 1)), draw(st.integers(0, 1))] = draw(st.sampled_from(rc._POKE_CPLX))
        frac, acc = rc._bits(draw, {"bits"} if why == "bits" else set())
        stage = OUT_U8_SAT if why == "stage" else OUT_I32
        rows = draw(st.integers(2, 6) if why == "shape" else st.one_of(st.just(1), st.integers(2, 6)))
        cap = min(PROPERTY_MAX_WIDTH, PROPERTY_MAX_FRAMES // rows)
        G = tiles_per_group(D) if 2 <= D <= MAX_D else 1
        edges = [4, 64, 256, W * D, T * D // 2, T * D, G * T * D]
        width = draw(st.one_of(st.integers(1, 64), st.integers(1, cap),
                               st.tuples(st.sampled_from(edges), st.sampled_from([-1, 0, 1, D, -D, phase])).map(sum)))
        width = max(1, min(width, cap))
        if why == "shape":
            width += width % ROW_UNIT == 0
        elif rows > 1:
            width = max(ROW_UNIT, width // ROW_UNIT * ROW_UNIT)
        x_lead = draw(st.sampled_from([2, 4, 6, 8, 12, 20]) if why == "align" else st.sampled_from([0, 0, 16, 32, 48, 496]))
        y_lead = draw(st.integers(0, 15)) * (4 if stage == OUT_I32 else 1)  # y at any element address
        src = rc.Case("cplx", "fast", "i16", 2, stage, 1, D, phase, tuple((int(a), int(b)) for a, b in h), frac, acc, rows,
                      width, draw(rc._SEED), draw(st.sampled_from(["uniform", "uniform", "ends", "min", "max"])), x_lead, y_lead)
        assert math.prod((rows, width)) <= PROPERTY_MAX_FRAMES
        return why, src

    return case()
