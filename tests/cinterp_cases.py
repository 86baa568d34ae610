"""Reference, predicted dispatch and shapes of the interpolating complex-tap FIR
(include/fir_cinterp.h) -- a test helper, not a test module.

``want``: what fir_cplx_interp_rows must give.  The contract is "exactly what fir_cplx_rows gives for
x zero-stuffed by U", and fir_cplx_rows' reference is tests/cplx_ref.py's ``want`` (two real filters
of the committed C oracle); so this is that function on ``stuffed(x, U)``.  ``want_loop`` is the
header's polyphase formula in plain Python ints, written without a stuffed signal: the only reference
once a sum can pass 2^63; tests/test_cinterp_cases.py holds the first against the second, and the
second against ``cplx_ref.cplx_loop`` of the stuffed signal.

``predicted_route``: the kernel a call takes, written from the conditions the header documents, never
by asking the library.

The shape lists are in terms of the fast kernel's constants (csrc_cinterp/fir1d_cplx_interp.hip): a
workgroup owns F = 2048 input frames of one row and works through them as tiles of T = tile(U) frames;
a tile is computed in passes of PASS = 256 frames, lane u owning input frame u of each pass (so a
lane's run of input frames is 1 and a wave's run W = 64).
"""
from __future__ import annotations

import numpy as np

import cplx_ref

OUT_U8_SAT, OUT_I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)  # FIR_CINTERP_*
BUCKETS = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 33)
# kCiF, kBlock, kWave, a lane's frames per pass, kCiMaxU, kCiMaxTaps, kCiMaxPerPhase, kChunk (cext_device.h)
F, PASS, W, LANE, MAX_U, MAX_TAPS, MAX_PER_PHASE, ROW_UNIT = 2048, 256, 64, 1, 16, 128, 32, 4


def tile(U: int) -> int:
    """T: F halved while the tile's T * U * 8 output bytes exceed 16 KiB, not below 256."""
    T = F
    while T > 256 and T * U * 8 > 16384:
        T //= 2
    return T


def fast_max_taps(U: int) -> int:
    """The most taps the fast kernel takes at this U: 128, and 32 per phase."""
    return min(MAX_TAPS, MAX_PER_PHASE * U)


def window(L: int, U: int) -> int:
    """The header's W: input frames in the window all phases share."""
    lo = hi = None
    for e in range(U):
        pe, ce = (e + L // 2) % U, (e + L // 2) // U
        if pe >= L:
            continue
        ne = -(-(L - pe) // U)
        lo = ce - ne + 1 if lo is None else min(lo, ce - ne + 1)
        hi = ce if hi is None else max(hi, ce)
    return hi - lo + 1


def bucket(L: int, U: int) -> int:
    return min(b for b in BUCKETS if b >= window(L, U))


def stuffed(x: np.ndarray, U: int) -> np.ndarray:
    """x (last axis 2 * width interleaved values) with U - 1 zero frames after every frame."""
    x = np.asarray(x)
    width = x.shape[-1] // 2
    xu = np.zeros(x.shape[:-1] + (width * U, 2), x.dtype)
    xu[..., ::U, :] = x.reshape(x.shape[:-1] + (width, 2))
    return xu.reshape(x.shape[:-1] + (2 * width * U,))


def want(x, hq, U: int, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    return cplx_ref.want(stuffed(x, U), hq, frac, acc, stage)


def want_loop(x, hq, U: int, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    """The header's polyphase formula as plain Python ints (small inputs only): output frame
    i * U + e sums the taps p + U t, p = (e + L // 2) % U, over the frames i + c - t inside the row."""
    x = np.asarray(x, dtype=np.int16)
    h = [(int(a), int(b)) for a, b in np.asarray(hq, dtype=object).reshape(-1, 2)]
    L = len(h)
    x2 = x.reshape(-1, x.shape[-1])
    width = x2.shape[1] // 2
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)

    def finish(v: int) -> int:
        v &= mask
        if v & sign:
            v -= 1 << acc
        v = (v + bias) >> frac
        if stage == OUT_U8_SAT:
            return 0 if v < 0 else (255 if v > 255 else v)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the int32 stage keeps the low 32 bits

    out = np.zeros((x2.shape[0], 2 * width * U), np.uint8 if stage == OUT_U8_SAT else np.int32)
    for r in range(x2.shape[0]):
        row = [int(v) for v in x2[r]]
        for i in range(width):
            for e in range(U):
                p, c = (e + L // 2) % U, (e + L // 2) // U
                re = im = 0
                n = -(-(L - p) // U) if p < L else 0  # the phase's taps: t in [0, n)
                # ... of which frame f = i + c - t lies in the row: 0 <= f < width (the loop is then
                # as long as the row at most, whatever the tap count)
                for t in range(max(0, i + c - width + 1), min(n, i + c + 1)):
                    f = i + c - t
                    hr, hi = h[p + U * t]
                    re += hr * row[2 * f] - hi * row[2 * f + 1]
                    im += hr * row[2 * f + 1] + hi * row[2 * f]
                out[r, 2 * (i * U + e)], out[r, 2 * (i * U + e) + 1] = finish(re), finish(im)
    return out.reshape(x.shape[:-1] + (2 * width * U,))


def _parts(hq) -> np.ndarray:
    """The 2 * taps tap parts as a flat int64 array (they fit in int32)."""
    return np.asarray(hq).astype(np.int64).reshape(-1)


def sum_can_pass_2_63(hq) -> bool:
    """The restated needs_wide bound: sum_k (|hr[k]| + |hi[k]|) * 32768 could reach 2^63."""
    return int(np.abs(_parts(hq)).sum()) * 32768 >= 1 << 63  # the int64 sum is at most 2^31 * 2^31


def predicted_route(x_addr: int, y_addr: int, rows: int, width: int, hq, U: int, frac: int = 12, acc: int = 32,
                    stage: int = OUT_I32) -> tuple:
    """(route, window bucket) from the header's "Dispatch" section; y may sit at any element address."""
    if rows == 0 or width == 0:
        return NONE, 0
    parts = _parts(hq)
    L = len(parts) // 2
    dot2 = int(np.abs(parts).max()) <= 32767 and acc <= 32 and frac <= 31
    groups = -(-width // F)
    if (dot2 and 2 <= U <= MAX_U and L <= MAX_TAPS and -(-L // U) <= MAX_PER_PHASE and stage == OUT_I32
            and x_addr % 16 == 0 and (rows == 1 or width % ROW_UNIT == 0) and width < 1 << 40 and rows * groups < 1 << 31):
        return FAST, bucket(L, U)
    if dot2 and x_addr % 4 == 0:
        return GENERIC32, 0
    if acc >= 64 and sum_can_pass_2_63(hq):
        return GENERIC128, 0
    return GENERIC64, 0


# ---- shapes ----------------------------------------------------------------------------------------
def edge_widths(U: int) -> list:
    """Input widths one below, at and one past: 1 frame, a lane's run (LANE = 1, the same), a wave's
    run (W), a pass (PASS), a tile (T), a workgroup (F) and two workgroups (2 F)."""
    marks = (1, LANE, W, PASS, tile(U), F, 2 * F)
    return sorted({m + d for m in marks for d in (-1, 0, 1) if m + d >= 1})


def multi_row_shapes(U: int) -> list:
    """(rows, width): rows of a multiple of 4 frames, from rows far narrower than a window to rows of
    one workgroup's frames and one chunk more; (5, 2 * T + 4) and (3, F + 4) leave the row's last
    workgroup (and its last tile) partly empty."""
    return [(3, 4), (5, 8), (7, 12), (300, 4), (2, F), (3, F + 4), (5, tile(U) + 4), (9, 252)]


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
WHY = ("", "", "", "", "", "", "", "rate", "taps", "value", "bits", "stage", "shape", "align")
PROPERTY_MAX_TAPS, PROPERTY_MAX_PRODUCT = 140, 20000  # input frames * U of a case, at most


def property_case():
    from hypothesis import strategies as st

    import rate_property_cases as rc

    @st.composite
    def case(draw):
        why = WHY[(draw(rc._SEED) * 2654435761 % 2**32 * len(WHY)) >> 32]  # hashed, as rc._route_and_reasons
        U = draw(st.one_of(st.just(1), rc._ABOVE_RATE) if why == "rate" else rc._IN_RATE)
        lmax = fast_max_taps(U) if 2 <= U <= MAX_U else MAX_TAPS
        if why == "taps":  # too many per phase where 32 U < 128, too many in all otherwise
            L = draw(st.one_of(st.just(lmax + 1), st.integers(lmax + 1, PROPERTY_MAX_TAPS)))
        else:
            near = sorted({min(lmax, max(1, (b - d) * U + k)) for b in BUCKETS for d in (0, 1) for k in (-1, 0, 1)})
            L = draw(st.one_of(st.integers(1, 9), st.integers(1, max(1, U)), st.integers(1, lmax), st.sampled_from(near),
                               st.sampled_from([lmax, max(1, lmax - 1)])))
        kinds = ["q412", "q412", "small", "int16", "ends"] + (["mad24", "wide"] if why == "value" else [])
        h = rc._zero_some(draw, rc._tap_values(draw, 2 * L, kinds, -32767), 2 * U).reshape(L, 2)  # one whole phase
        if draw(st.integers(0, 7)) == 0:
            h[:, draw(st.integers(0, 1))] = 0  # purely real or purely imaginary taps
        if why == "value":  # whatever the kind drew, one part is outside [-32767, 32767]
            h[draw(st.integers(0, L - 1)), draw(st.integers(0, 1))] = draw(st.sampled_from(rc._POKE_CPLX))
        frac, acc = rc._bits(draw, {"bits"} if why == "bits" else set())
        stage = OUT_U8_SAT if why == "stage" else OUT_I32
        rows = draw(st.integers(2, 6) if why == "shape" else st.one_of(st.just(1), st.integers(2, 6)))
        cap = PROPERTY_MAX_PRODUCT // (rows * U)  # at least 83: 6 rows at U = 40
        T = tile(U) if 2 <= U <= MAX_U else 256
        edges = [4, W, PASS, T, F, 2 * F]
        width = draw(st.one_of(st.integers(1, 64), st.integers(1, cap),
                               st.tuples(st.sampled_from(edges), st.sampled_from([-1, 0, 1, 4, -4])).map(sum)))
        width = max(1, min(width, cap))
        if why == "shape":
            width -= width % ROW_UNIT == 0  # a multiple of 4 is at least 4
        elif rows > 1:
            width = max(ROW_UNIT, width // ROW_UNIT * ROW_UNIT)
        x_lead = draw(st.sampled_from([2, 4, 6, 8, 12, 20]) if why == "align" else st.sampled_from([0, 0, 16, 32, 48, 496]))
        y_lead = draw(st.integers(0, 15)) * (4 if stage == OUT_I32 else 1)  # y at any element address
        src = rc.Case("cplx", "fast", "i16", 2, stage, U, 1, 0, tuple((int(a), int(b)) for a, b in h), frac, acc, rows,
                      width, draw(rc._SEED), draw(st.sampled_from(["uniform", "uniform", "ends", "min", "max"])), x_lead, y_lead)
        assert rows * width * U <= PROPERTY_MAX_PRODUCT
        return why, src

    return case()
