"""Reference, predicted dispatch and shapes of the rational resampling complex-tap FIR
(include/fir_cresample.h) -- a test helper, not a test module.

``want``: what fir_cplx_resample_rows must give.  The contract is ``y[r, m, :] = y_up[r, m * D + phase, :]``
with y_up what fir_cplx_interp_rows gives, whose reference is tests/cinterp_cases.py's ``want`` (two
real filters of the committed C oracle on the zero-stuffed signal); so this is that array viewed as
frames and sliced ``[:, phase::D]``.  ``want_loop`` is the header's polyphase formula in plain Python
ints, written without a stuffed signal or an intermediate: the only reference once a sum can pass
2^63; tests/test_cresample_cases.py holds the first against the second.

``predicted_route``: the kernel a call takes, written from the conditions the header documents, never
by asking the library.

The shape lists are in terms of the fast kernel's constants (csrc_cresample/fir1d_cplx_resample.hip):
one PERIOD is D input frames and U output frames; a workgroup owns P = periods(D) periods of one row
and works through them as tiles of T = tile(U, D) periods; a tile is computed in passes of PASS = 256
periods, lane u owning period u of each pass (so a lane's run of output frames is U and a wave's run
W * U).
"""
from __future__ import annotations

import numpy as np

import cinterp_cases

OUT_U8_SAT, OUT_I32 = 0, 1
NONE, FAST, GENERIC32, GENERIC64, GENERIC128 = range(5)  # FIR_CRESAMPLE_*
BUCKETS = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32)
# kBlock, kWave, kCrMaxUD, kCrMaxTaps, kCrMaxNP, kChunk (csrc_cext/cext_device.h)
PASS, W, MAX_UD, MAX_TAPS, MAX_PER_PHASE, ROW_UNIT = 256, 64, 16, 128, 32, 4


def periods(D: int) -> int:
    """P: 256 doubled until P * D * 4 input bytes reach 4 KiB."""
    P = 256
    while P * D * 4 < 4096:
        P *= 2
    return P


def tile(U: int, D: int) -> int:
    """T: P halved while the tile's T * U * 8 output bytes exceed 16 KiB, not below 256."""
    T = periods(D)
    while T > 256 and T * U * 8 > 16384:
        T //= 2
    return T


def fast_max_taps(U: int) -> int:
    """The most taps the fast kernel takes at this U: 128, and 32 per phase."""
    return min(MAX_TAPS, MAX_PER_PHASE * U)


def out_width(width: int, U: int, D: int, phase: int) -> int:
    return len(range(phase, width * U, D))


def phases(L: int, U: int, D: int, phase: int) -> list:
    """(p_q, c_q, n_q) of the header for q = 0 .. U - 1."""
    out = []
    for q in range(U):
        a = phase + L // 2 + q * D
        p, c = a % U, a // U
        out.append((p, c, -(-(L - p) // U) if p < L else 0))
    return out


def bucket(L: int, U: int, D: int, phase: int) -> int:
    """The header's tap bucket: the smallest that holds the longest sub-filter (1 when all are empty)."""
    need = max(n for _, _, n in phases(L, U, D, phase))
    return min(b for b in BUCKETS if b >= need)


def sliced(full: np.ndarray, D: int, phase: int) -> np.ndarray:
    frames = full.reshape(full.shape[:-1] + (full.shape[-1] // 2, 2))[..., phase::D, :]
    return np.ascontiguousarray(frames).reshape(full.shape[:-1] + (-1,))


def want(x, hq, U: int, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    return sliced(cinterp_cases.want(x, hq, U, frac, acc, stage), D, phase)


def want_loop(x, hq, U: int, D: int, phase: int = 0, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    """The header's polyphase formula as plain Python ints (small inputs only): output frame
    m = v * U + q sums the taps p_q + U t over the frames v * D + c_q - t inside the row."""
    x = np.asarray(x, dtype=np.int16)
    h = [(int(a), int(b)) for a, b in np.asarray(hq, dtype=object).reshape(-1, 2)]
    L = len(h)
    x2 = x.reshape(-1, x.shape[-1])
    width = x2.shape[1] // 2
    ow = out_width(width, U, D, phase)
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)

    def finish(v: int) -> int:
        v &= mask
        if v & sign:
            v -= 1 << acc
        v = (v + bias) >> frac
        if stage == OUT_U8_SAT:
            return 0 if v < 0 else (255 if v > 255 else v)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the int32 stage keeps the low 32 bits

    ph = phases(L, U, D, phase)
    out = np.zeros((x2.shape[0], 2 * ow), np.uint8 if stage == OUT_U8_SAT else np.int32)
    for r in range(x2.shape[0]):
        row = [int(v) for v in x2[r]]
        for m in range(ow):
            v, q = divmod(m, U)
            p, c, n = ph[q]
            top = v * D + c  # tap p + U t meets frame top - t
            re = im = 0
            # the phase's taps t in [0, n) whose frame lies in the row: 0 <= top - t < width
            for t in range(max(0, top - width + 1), min(n, top + 1)):
                f = top - t
                hr, hi = h[p + U * t]
                re += hr * row[2 * f] - hi * row[2 * f + 1]
                im += hr * row[2 * f + 1] + hi * row[2 * f]
            out[r, 2 * m], out[r, 2 * m + 1] = finish(re), finish(im)
    return out.reshape(x.shape[:-1] + (2 * ow,))


def _parts(hq) -> np.ndarray:
    """The 2 * taps tap parts as a flat int64 array (they fit in int32)."""
    return np.asarray(hq).astype(np.int64).reshape(-1)


def sum_can_pass_2_63(hq) -> bool:
    """The restated needs_wide bound: sum_k (|hr[k]| + |hi[k]|) * 32768 could reach 2^63."""
    return int(np.abs(_parts(hq)).sum()) * 32768 >= 1 << 63  # the int64 sum is at most 2^31 * 2^31


def predicted_route(x_addr: int, y_addr: int, rows: int, width: int, hq, U: int, D: int, phase: int = 0,
                    frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> tuple:
    """(route, tap bucket) from the header's "Dispatch" section; y may sit at any element address."""
    ow = -(-(width * U - phase) // D) if width * U > phase else 0  # out_width, without a range of that length
    if rows == 0 or ow == 0:
        return NONE, 0
    parts = _parts(hq)
    L = len(parts) // 2
    dot2 = int(np.abs(parts).max()) <= 32767 and acc <= 32 and frac <= 31
    if (dot2 and 2 <= U <= MAX_UD and 2 <= D <= MAX_UD and L <= MAX_TAPS and -(-L // U) <= MAX_PER_PHASE
            and stage == OUT_I32 and x_addr % 16 == 0 and (rows == 1 or width % ROW_UNIT == 0) and width < 1 << 40
            and rows * -(-ow // (periods(D) * U)) < 1 << 31):
        return FAST, bucket(L, U, D, phase)
    if dot2 and x_addr % 4 == 0:
        return GENERIC32, 0
    if acc >= 64 and sum_can_pass_2_63(hq):
        return GENERIC128, 0
    return GENERIC64, 0


# ---- shapes ----------------------------------------------------------------------------------------
def edge_out_widths(U: int, D: int) -> list:
    """Output frames at which something ends: 1 frame, a lane's run (U), a wave's run (W U), a pass
    (PASS U), a tile (T U), a workgroup (P U) and two workgroups (2 P U)."""
    return sorted({1, U, W * U, PASS * U, tile(U, D) * U, periods(D) * U, 2 * periods(D) * U})


def edge_widths(U: int, D: int) -> list:
    """Input widths ceil(edge * D / U), one less and one more, for every edge of edge_out_widths: the
    row's last output frame lies one below, at or one past the edge."""
    return sorted({-(-e * D // U) + d for e in edge_out_widths(U, D) for d in (-1, 0, 1) if -(-e * D // U) + d >= 1})


def multi_row_shapes(U: int, D: int) -> list:
    """(rows, width): rows of a multiple of 4 frames, from rows far narrower than a window to rows of
    one workgroup's frames and one chunk more; (5, T D + 4) leaves the last tile partly empty."""
    P, T = periods(D), tile(U, D)
    return [(300, 4), (3, 4), (5, 8), (7, 12), (2, P * D), (3, P * D + 4), (5, T * D + 4), (9, 252)]


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
WHY = ("",) * 8 + ("rate U", "rate D", "taps", "value", "bits", "stage", "shape", "align")
PROPERTY_MAX_TAPS, PROPERTY_MAX_PRODUCT = 140, 20000  # input frames * U of a case, at most


def property_case():
    from hypothesis import strategies as st

    import rate_property_cases as rc

    @st.composite
    def case(draw):
        why = WHY[(draw(rc._SEED) * 2654435761 % 2**32 * len(WHY)) >> 32]  # hashed, as rc._route_and_reasons
        U = draw(st.one_of(st.just(1), rc._ABOVE_RATE) if why == "rate U" else rc._IN_RATE)
        D = draw(st.one_of(st.just(1), rc._ABOVE_RATE) if why == "rate D" else rc._IN_RATE)
        phase = draw(st.one_of(st.just(0), st.just(D - 1), st.integers(0, D - 1)))
        lmax = fast_max_taps(U) if 2 <= U <= MAX_UD else MAX_TAPS
        if why == "taps":  # too many per phase where 32 U < 128, too many in all otherwise
            L = draw(st.one_of(st.just(lmax + 1), st.integers(lmax + 1, PROPERTY_MAX_TAPS)))
        else:
            near = sorted({min(lmax, max(1, b * U + k)) for b in BUCKETS for k in (-1, 0, 1)})
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
        if 2 <= U <= MAX_UD and 2 <= D <= MAX_UD:
            edges = [4] + [-(-e * D // U) for e in edge_out_widths(U, D)]
        else:
            edges = [4, W, PASS, 2 * PASS]
        width = draw(st.one_of(st.integers(1, 64), st.integers(1, cap),
                               st.tuples(st.sampled_from(edges), st.sampled_from([-1, 0, 1, 4, -4])).map(sum)))
        width = max(1, min(width, cap))
        if why == "shape":
            width -= width % ROW_UNIT == 0  # a multiple of 4 is at least 4
        elif rows > 1:
            width = max(ROW_UNIT, width // ROW_UNIT * ROW_UNIT)
        if width * U <= phase:  # nothing to compute: not a case of any route
            phase = 0
        x_lead = draw(st.sampled_from([2, 4, 6, 8, 12, 20]) if why == "align" else st.sampled_from([0, 0, 16, 32, 48, 496]))
        y_lead = draw(st.integers(0, 15)) * (4 if stage == OUT_I32 else 1)  # y at any element address
        src = rc.Case("cplx", "fast", "i16", 2, stage, U, D, phase, tuple((int(a), int(b)) for a, b in h), frac, acc, rows,
                      width, draw(rc._SEED), draw(st.sampled_from(["uniform", "uniform", "ends", "min", "max"])), x_lead, y_lead)
        assert rows * width * U <= PROPERTY_MAX_PRODUCT
        return why, src

    return case()
