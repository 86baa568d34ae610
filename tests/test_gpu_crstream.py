"""GPU: the streaming U/D resampling complex-tap FIR with carried history (fir_cplx_rstream_block_dev of
libfir_crstream.so, through fir_hip.torch_crstream).

The reference for every value is tests/crstream_cases.py's ``want_block`` (identity 2 of
include/fir_crstream.h over tests/cinterp_cases.py's ``want``, the committed C oracle;
tests/test_crstream_cases.py holds it against Python-int loops), so every comparison is
np.array_equal, no tolerance: y, hist_out and next_phase.  Every call asserts that the FIR kernel it
launched (last_launch) is what the library's route query says, and that both are what
predicted_route works out from the header's "Routes" section.  x, hist_in, y and hist_out all sit
inside larger allocations between hostile samples and canaries (tests/guarded.py).  No test here
provokes a fault: all buffers are in bounds.

The fast kernel is the one-shot resampler's (tests/test_gpu_cresample.py's docstring has its geometry:
a workgroup owns P periods of D input and U output frames, in tiles of T periods, staging in 16-byte
chunks from the boundary at or below its first window) with a causal plan and a history read in the
staging branch for chunks not wholly inside the block.  So the shapes here are the tile's and the
workgroup's output edges, the block's start (widths below, at and past H, the first chunk across
frame 0 at every lead), and splits of one signal into blocks of one frame, a few frames, up to a
workgroup's input, and multiples of D.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import cresample_cases as cr
import crstream_cases as rs
import fir_hip
import rate_property_cases as rc
from fir_hip import crstream, torch_crstream
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT
RATES = [(3, 2), (2, 3), (4, 3), (16, 15), (2, 16), (16, 2)]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at {tuple(int(v) for v in bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _launch(xd, hd, hod, yd, taps, U, D, phase, frac, acc, stage, what, route=None, stream=None):
    """One call on device tensors that already sit in guarded buffers: predicted route == the
    library's route query == what was launched.  Returns the prediction."""
    rows = xd.numel() // xd.shape[-1] if xd.shape[-1] else int(np.prod(xd.shape[:-1], dtype=np.int64))
    width = xd.shape[-1] // 2
    addrs = (xd.data_ptr(), 0 if hd is None else hd.data_ptr(), yd.data_ptr(), 0 if hod is None else hod.data_ptr())
    pred = rs.predicted_route(*addrs, rows, width, taps.h, U, D, phase, frac, acc, stage)
    if route is not None:
        assert pred[0] == route, (what, pred)
    assert tuple(crstream.route(*addrs, rows, width, taps.h, U, D, phase, frac, acc, stage)) == pred, what
    out = torch_crstream.fir1d_fixed_rows_cplx_resample_block_dev(xd, hd, hod, taps, U, D, phase, frac, acc, stage, out=yd,
                                                                  stream=stream)
    assert out is yd
    assert tuple(crstream.last_launch()) == pred, (what, crstream.last_launch(), pred)
    return pred


def _check(x, hist, hq, U, D, phase=0, frac=12, acc=32, stage=I32, *, route=None, ref=None, x_lead=0, y_lead=0, hi_lead=0,
           ho_lead=0, what=""):
    """One block on guarded buffers against want_block (or ``ref``): y, hist_out, the guards."""
    rows, width = x.shape[0], x.shape[1] // 2
    taps = hq if isinstance(hq, torch_crstream.CplxTaps) else torch_crstream.CplxTaps(hq)
    want_y, want_h, want_p = ref if ref is not None else rs.want_block(x, hist, taps.h, U, D, phase, frac, acc, stage)
    assert want_y.shape == (rows, 2 * rs.out_width(width, U, D, phase)), what
    assert want_h.shape == (rows, 2 * rs.hist_frames(taps.n, U)), what
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    hd = None if hist is None else guarded_input(torch.from_numpy(hist), lead_bytes=hi_lead, device=DEV)
    yd, y_guards = guarded_output(want_y.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=y_lead, device=DEV)
    hod, h_guards = guarded_output(want_h.shape, torch.int16, lead_bytes=ho_lead, device=DEV)
    pred = _launch(xd, hd, hod, yd, taps, U, D, phase, frac, acc, stage, what, route)
    assert crstream.next_phase(width, U, D, phase) == want_p == crstream.lib().fir_cplx_rstream_next_phase(width, U, D, phase), what
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), want_y, (what, "y"))
    if want_h.shape[1]:
        _same(hod.cpu().numpy(), want_h, (what, "hist_out"))
    y_guards(f"{what} y")
    h_guards(f"{what} hist_out")
    return pred


def _taps_for(U, need):
    """A tap count whose longest sub-filter has `need` taps (bucket `need`), or None past 128 taps."""
    L = U if need == 1 else need * U - 1
    return L if L <= rs.MAX_TAPS else None


# ---- 1. one block per rate, zero and hostile history -------------------------------------------------
def test_the_tap_counts_of_test_1_reach_the_buckets_1_4_16_and_32():
    hit = {rs.bucket(L, U, D, ph) for U, D in RATES for need in (1, 4, 16, 32) for L in [_taps_for(U, need)] if L
           for ph in (0, D - 1)}
    assert hit >= {1, 4, 16, 32}


@pytest.mark.parametrize("U,D", RATES)
def test_one_block_zero_and_hostile_history(U, D):
    rng = np.random.default_rng(100 * U + D)
    widths = rs.edge_widths(U, D)  # out_width 1, and around T U and P U
    ows = [rs.out_width(w, U, D, 0) for w in widths]
    for e in (rs.tile(U, D) * U, rs.periods(D) * U):
        assert ows[0] >= 1 and any(e - U <= o <= e for o in ows) and any(e < o <= e + U for o in ows), (e, ows)
    for need in (1, 4, 16, 32):
        L = _taps_for(U, need)
        if L is None:
            continue
        H = rs.hist_frames(L, U)
        taps = torch_crstream.CplxTaps(rs.taps(rng, L))
        for k, width in enumerate(widths):
            x = rs.frames(rng, 1, width)
            for phase in (0, D - 1):
                # both histories at the edges of the first and last width, one of them in between
                hists = (None, rs.hostile_history(rng, 1, H)) if k in (0, len(widths) - 1) else ((None,) if (k + phase) % 2 else (rs.hostile_history(rng, 1, H),))
                for hist in hists:
                    got = _check(x, hist, taps, U, D, phase, what=(U, D, L, phase, width, hist is None))
                    want = (rs.FAST, rs.bucket(L, U, D, phase)) if width * U > phase else (rs.NONE, 0)
                    assert got == want


# ---- 2. the block start ------------------------------------------------------------------------------
def test_the_block_start():
    """Widths below, at and past H, so that hist_out mixes hist_in and x; phase >= width * U (no output,
    the history still written); and the workgroup's first 16-byte chunk across frame 0 at every lead:
    the lowest window of period 0 starts at frame S <= 0, and S mod 4 takes its four values."""
    rng = np.random.default_rng(200)
    leads = set()
    for U, D, L, phases in ((3, 2, 11, (0, 1)), (3, 2, 47, (0, 1)), (2, 3, 8, (0, 2)), (2, 3, 13, (1, 2)), (4, 3, 63, (0, 2)),
                            (16, 15, 128, (0, 14)), (2, 16, 64, (0, 15)), (16, 2, 60, (0, 1)), (4, 3, 3, (0, 1, 2))):
        H = rs.hist_frames(L, U)
        taps = torch_crstream.CplxTaps(rs.taps(rng, L))
        for phase in phases:
            S = rs.window_start(L, U, D, phase)
            assert -H <= S
            leads.add(S % 4)
            for width in sorted({1, 2, 3, max(1, H - 1), max(1, H), H + 1, 4, 5, 8}):
                x = rs.frames(rng, 1, width)
                for hist in (None, rs.hostile_history(rng, 1, H)):
                    want = (rs.FAST, rs.bucket(L, U, D, phase)) if width * U > phase else (rs.NONE, 0)
                    assert _check(x, hist, taps, U, D, phase, what=(U, D, L, phase, width, hist is None)) == want
    assert leads == {0, 1, 2, 3}
    # phase >= width * U: no output frame, the history still moves
    taps = torch_crstream.CplxTaps(rs.taps(rng, 64))
    for width in (1, 2, 7):
        x, hist = rs.frames(rng, 1, width), rs.hostile_history(rng, 1, 31)
        assert width * 2 <= 15 and _check(x, hist, taps, 2, 16, 15, what=("no output", width)) == (rs.NONE, 0)


# ---- 3. split invariance on the device ---------------------------------------------------------------
def _splits(rng, N, D, P):
    return {
        "one-frame blocks": [1] * 150 + [N - 150],
        "widths in [0, 3 D]": [0, 0] + rs.random_split(rng, N, 3 * D),
        "up to a workgroup's input": rs.random_split(rng, N, P * D),
        "multiples of D": [D * w for w in rs.random_split(rng, N // D, 3 * P // 2)] + ([N % D] if N % D else []),
    }


@pytest.mark.parametrize("U,D,L", [(3, 2, 72), (16, 15, 100)])
def test_split_invariance_one_row(U, D, L):
    """One row of 2 P D + 37 frames cut four ways; every block reads its frames in place, out of ONE
    guarded copy of the row (its neighbours are the frames before and after it), and writes its kept
    frames in place into one guarded output; the histories ping-pong between two guarded buffers.
    Compared with one call over the whole signal and with want_block, final history and phase included."""
    rng = np.random.default_rng(300 + U)
    P = rs.periods(D)
    N = 2 * P * D + 37
    H = rs.hist_frames(L, U)
    taps = torch_crstream.CplxTaps(rs.taps(rng, L))
    x, hist0 = rs.frames(rng, 1, N), rs.hostile_history(rng, 1, H)
    for hist, phase0 in ((hist0, D - 1), (None, 0)):
        want_y, want_h, want_p = rs.want_block(x, hist, taps.h, U, D, phase0)
        assert _check(x, hist, taps, U, D, phase0, ref=(want_y, want_h, want_p), what=("whole", U, D))[0] == rs.FAST
        for name, widths in _splits(rng, N, D, P).items():
            assert sum(widths) == N
            xd = guarded_input(torch.from_numpy(x), device=DEV)
            yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
            hb, hg = zip(*(guarded_output((1, 2 * H), torch.int16, device=DEV) for _ in range(2)))
            cur, at, done, phase, routes = None, 0, 0, phase0, set()
            if hist is not None:
                hb[0].copy_(torch.from_numpy(hist))
                cur = 0
            for w in widths:
                ow = rs.out_width(w, U, D, phase)
                nxt = 1 if cur is None else 1 - cur
                routes.add(_launch(xd[:, 2 * at:2 * (at + w)], None if cur is None else hb[cur], hb[nxt],
                                   yd[:, 2 * done:2 * (done + ow)], taps, U, D, phase, 12, 32, I32, (name, at, w))[0])
                phase, at, done, cur = crstream.next_phase(w, U, D, phase), at + w, done + ow, nxt
            torch.cuda.synchronize()
            assert phase == want_p and 2 * done == want_y.shape[1], name
            _same(yd.cpu().numpy(), want_y, (U, D, name, "y"))
            _same(hb[cur].cpu().numpy(), want_h, (U, D, name, "hist_out"))
            y_guards(name)
            for g in hg:
                g(name)
            assert routes <= {rs.FAST, rs.GENERIC32, rs.NONE} and rs.FAST in routes, (name, routes)


@pytest.mark.parametrize("U,D,L", [(3, 2, 72), (4, 3, 64)])
def test_split_invariance_rows(U, D, L):
    """3 rows, blocks of a multiple of 4 frames: every block is FAST, each on its own guarded buffers."""
    rng = np.random.default_rng(350 + U)
    P = rs.periods(D)
    N = (2 * P * D + 37) // 4 * 4
    rows = 3
    taps = torch_crstream.CplxTaps(rs.taps(rng, L))
    x, hist = rs.frames(rng, rows, N), rs.hostile_history(rng, rows, rs.hist_frames(L, U))
    one = rs.want_block(x, hist, taps.h, U, D, D - 1)
    assert _check(x, hist, taps, U, D, D - 1, ref=one, what=("whole", U, D))[0] == rs.FAST
    for name, widths in (("4-frame blocks", [4] * 20 + [N - 80]),
                         ("up to a workgroup's input", [4 * w for w in rs.random_split(rng, N // 4, P * D // 4)]),
                         ("multiples of 4 D", [4 * D * w for w in rs.random_split(rng, N // (4 * D), P // 2)] + [N % (4 * D)])):
        ys, at, h, phase = [], 0, hist, D - 1
        for w in widths:
            xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
            ref = rs.want_block(xb, h, taps.h, U, D, phase)
            got = _check(xb, h, taps, U, D, phase, ref=ref, what=(U, D, name, at, w))
            assert got[0] == (rs.FAST if ref[0].size else rs.NONE), (name, at, w, got)
            ys.append(ref[0])
            at, h, phase = at + w, ref[1], ref[2]
        # the per-block references chain to the single-block one (the device equalled each of them)
        _same(np.concatenate(ys, axis=1), one[0], (U, D, name, "y"))
        _same(h, one[1], (U, D, name, "hist_out"))
        assert phase == one[2]


# ---- 4. generic routes -------------------------------------------------------------------------------
def _three_blocks(x, hist, hq, U, D, phase, widths, frac=12, acc=32, stage=I32, *, route, block=rs.want_block, what="", **leads):
    at, one = 0, block(x, hist, hq, U, D, phase, frac, acc, stage)
    ys = []
    for w in widths:
        xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
        ref = block(xb, hist, hq, U, D, phase, frac, acc, stage)
        _check(xb, hist, hq, U, D, phase, frac, acc, stage, ref=ref, route=route if ref[0].size else rs.NONE, what=(what, at, w),
               **leads)
        ys.append(ref[0])
        at, hist, phase = at + w, ref[1], ref[2]
    assert at == x.shape[1] // 2
    _same(np.concatenate(ys, axis=1), one[0], (what, "chained y"))
    _same(hist, one[1], (what, "chained hist"))
    assert phase == one[2]


def test_generic_routes_across_three_blocks():
    rng = np.random.default_rng(400)
    g32, g64 = rs.GENERIC32, rs.GENERIC64
    for rows, widths in ((1, (300, 3, 500)), (3, (260, 0, 40)), (2, (5, 1, 200))):
        x = rs.frames(rng, rows, sum(widths))

        def run(hq, U, D, phase, *a, route, what, **k):
            h = rs.hostile_history(rng, rows, rs.hist_frames(len(hq), U))
            for hist in (h, None):
                _three_blocks(x, hist, hq, U, D, phase, widths, *a, route=route, what=(what, rows, hist is None), **k)

        run(rs.taps(rng, 9, -40, 41), 3, 2, 1, 6, 32, U8, route=g32, what="u8 stage")
        run(rs.taps(rng, 40), 17, 5, 4, route=g32, what="U = 17")
        run(rs.taps(rng, 20), 3, 17, 16, route=g32, what="D = 17")
        run(rs.taps(rng, 16), 1, 3, 2, route=g32, what="U = 1")
        run(rs.taps(rng, 16), 3, 1, 0, route=g32, what="D = 1")
        run(rs.taps(rng, 12), 4, 3, 2, 12, 64, route=g64, what="acc 64")
        run(rs.taps(rng, 12), 4, 3, 0, route=g64, what="hist_out 2 bytes off 4", ho_lead=2)
        run(rs.taps(rng, 3), 4, 3, 0, route=None, what="H = 0: the histories' addresses do not matter", ho_lead=2, hi_lead=2)


def test_generic128_across_three_blocks():
    """needs_wide: 2^16 + 9 complex taps of +-(2^31 - 1) make sum(|hr| + |hi|) * 32768 pass 2^63, so the
    kernel sums in 128 bits.  The reference is want_block_loop (Python ints over the kept frames), so
    the blocks are a few frames."""
    rng = np.random.default_rng(463)
    L = (1 << 16) + 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert rs.sum_can_pass_2_63(hq)
    x = rs.frames(rng, 2, 9)
    for hist in (rs.hostile_history(rng, 2, rs.hist_frames(L, 3)), None):
        for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
            _three_blocks(x, hist, hq, 3, 2, 1, (4, 1, 4), frac, acc, stage, route=rs.GENERIC128, block=rs.want_block_loop,
                          what=("wide", frac, acc, hist is None))


# ---- 5. hist_out = None; taps <= up ------------------------------------------------------------------
def test_no_hist_out_writes_nothing_and_no_history_ignores_both():
    rng = np.random.default_rng(500)
    for L, U, D, rows, width in ((72, 3, 2, 1, 700), (20, 4, 3, 3, 260), (9, 2, 5, 4, 132)):
        H = rs.hist_frames(L, U)
        x, hist, hq = rs.frames(rng, rows, width), rs.hostile_history(rng, rows, H), rs.taps(rng, L)
        taps = torch_crstream.CplxTaps(hq)
        want_y, _, _ = rs.want_block(x, hist, hq, U, D, 1)
        xd, hd = guarded_input(torch.from_numpy(x), device=DEV), guarded_input(torch.from_numpy(hist), device=DEV)
        yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
        dummy, d_guards = guarded_output((rows, 2 * H), torch.int16, device=DEV)  # never passed: stays canary
        pred = _launch(xd, hd, None, yd, taps, U, D, 1, 12, 32, I32, ("no hist_out", L), route=rs.FAST)
        torch.cuda.synchronize()
        _same(yd.cpu().numpy(), want_y, ("no hist_out", L))
        y_guards("no hist_out y")
        d_guards("no hist_out dummy")
        assert bool((dummy.view(torch.uint8) == 0xA5).all()) and pred[1] == rs.bucket(L, U, D, 1)
    # taps <= up: H = 0, both history pointers are ignored (None, or empty tensors)
    for L, U, D, rows, width in ((3, 4, 3, 1, 901), (16, 16, 15, 4, 260), (1, 2, 2, 2, 64), (5, 17, 3, 2, 77)):
        assert rs.hist_frames(L, U) == 0
        x, hq = rs.frames(rng, rows, width), rs.taps(rng, L)
        want_y, want_h, _ = rs.want_block(x, None, hq, U, D, D - 1)
        assert want_h.shape == (rows, 0)
        xd = guarded_input(torch.from_numpy(x), device=DEV)
        yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
        pred = _launch(xd, None, None, yd, torch_crstream.CplxTaps(hq), U, D, D - 1, 12, 32, I32, ("no history", L, U))
        assert pred == ((rs.FAST, 1) if U <= 16 else (rs.GENERIC32, 0))
        torch.cuda.synchronize()
        _same(yd.cpu().numpy(), want_y, ("no history", L, U))
        y_guards("no history")
        _check(x, np.zeros((rows, 0), np.int16), hq, U, D, 0, what=("no history, empty tensors", L, U))
    # width = 0: the history is copied (zeros for None); rows of no frames
    for rows, L, U in ((1, 9, 2), (3, 72, 3)):
        hist, hq = rs.hostile_history(rng, rows, rs.hist_frames(L, U)), rs.taps(rng, L)
        for h in (hist, None):
            assert _check(np.zeros((rows, 0), np.int16), h, hq, U, 3, 2, what=("width 0", rows, L)) == (rs.NONE, 0)


# ---- 6. CplxResampleStream ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (2, 3)])
def test_stream_object(lead):
    rng = np.random.default_rng(600 + len(lead))
    L, U, D = 64, 4, 3
    H = rs.hist_frames(L, U)
    hq = rs.taps(rng, L)
    rows = int(np.prod(lead, dtype=np.int64))
    widths = [0, 1, 7, 1024, 0, 23, 3, 2048 + 4, 12, 5]
    N = sum(widths)
    x = rs.frames(rng, rows, N)
    s = torch_crstream.CplxResampleStream(hq, U, D, lead, phase=2, device=DEV)
    assert (s.phase, s.frames_in, s.frames_out) == (2, 0, 0) and s.history.shape == lead + (2 * H,)
    for rnd, (hist, phase) in enumerate(((None, 2), (rs.hostile_history(rng, rows, H), 1))):
        if rnd:
            s.reset(torch.from_numpy(hist.reshape(lead + (-1,))).to(DEV), phase)
            assert (s.phase, s.frames_in, s.frames_out) == (phase, 0, 0)
        want_y, want_h, want_p = rs.want_block(x, hist, hq, U, D, phase)
        ys, at = [], 0
        for w in widths:
            xb = guarded_input(torch.from_numpy(np.ascontiguousarray(x[:, 2 * at:2 * (at + w)]).reshape(lead + (2 * w,))), device=DEV)
            ys.append(s.push(xb))
            at += w
            assert s.frames_in == at and s.frames_out == rs.out_width(at, U, D, phase)
        torch.cuda.synchronize()
        got = torch.cat(ys, dim=-1).cpu().numpy().reshape(rows, -1)
        _same(got, want_y, ("stream", lead, rnd))
        _same(s.history.cpu().numpy().reshape(rows, -1), want_h, ("stream history", lead, rnd))
        assert s.phase == want_p
    s.reset()
    assert (s.phase, s.frames_in, s.frames_out) == (0, 0, 0) and not bool(s.history.any())
    with pytest.raises(fir_hip.FirHipError, match="leading axes"):
        s.push(torch.zeros(lead + (1, 8), dtype=torch.int16, device=DEV))
    with pytest.raises(fir_hip.FirHipError, match="up must be >= 1"):
        torch_crstream.CplxResampleStream(hq, 0, D, lead, device=DEV)


# ---- 7. graph capture --------------------------------------------------------------------------------
def test_two_blocks_are_captured_once_and_replayed():
    """The fast route allocates nothing and reads no device table: two consecutive blocks (history
    A -> B, then B -> A) captured into one graph on one side stream, a linear chain of four kernels,
    replayed once on a fresh pair of blocks and compared."""
    rng = np.random.default_rng(700)
    rows, U, D, phase, L = 4, 3, 2, 1, 72
    width = 1028
    H = rs.hist_frames(L, U)
    taps = torch_crstream.CplxTaps(rs.taps(rng, L))
    ow = rs.out_width(width, U, D, phase)
    assert rs.next_phase(width, U, D, phase) == phase and width % 4 == 0
    side = torch.cuda.Stream(device=DEV)
    xs = guarded_input(torch.zeros((2, rows, 2 * width), dtype=torch.int16), device=DEV)  # static input
    ys, y_guards = guarded_output((2, rows, 2 * ow), torch.int32, device=DEV)
    (ha, ga), (hb, gb) = (guarded_output((rows, 2 * H), torch.int16, device=DEV) for _ in range(2))
    bucket = rs.bucket(L, U, D, phase)

    def pair(what):
        for k, (hi, ho) in enumerate(((ha, hb), (hb, ha))):
            assert _launch(xs[k], hi, ho, ys[k], taps, U, D, phase, 12, 32, I32, (what, k), route=rs.FAST, stream=side) == (rs.FAST, bucket)

    with torch.cuda.stream(side):
        pair("warm-up")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pair("capture")
    torch.cuda.synchronize()
    hist0 = rs.hostile_history(rng, rows, H)
    blocks = [rs.frames(rng, rows, width) for _ in range(2)]
    want_y, want_h, _ = rs.want_block(np.concatenate(blocks, axis=1), hist0, taps.h, U, D, phase)
    ha.copy_(torch.from_numpy(hist0))
    xs.copy_(torch.from_numpy(np.stack(blocks)))
    ys.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _same(np.concatenate([ys[0].cpu().numpy(), ys[1].cpu().numpy()], axis=1), want_y, "replay")
    _same(ha.cpu().numpy(), want_h, "history after the replay")
    y_guards("graph y")
    ga("history A")
    gb("history B")


# ---- 8. random cases ---------------------------------------------------------------------------------
@settings(max_examples=40, **SETTINGS)
@given(cr.property_case(), st.integers(0, 2**32 - 1))
def test_random_splits_vs_oracle(case, seed):
    """tests/cresample_cases.property_case (taps, U, D, phase, rows, width, x and y leads, a reason off
    the fast route for about half the cases) cut into up to 5 blocks, the histories at drawn leads."""
    why, c = case
    rng = np.random.default_rng(seed)
    x = rc.samples(c)
    hq = np.asarray(c.hq, dtype=np.int64)
    taps = torch_crstream.CplxTaps(hq)
    H = rs.hist_frames(taps.n, c.up)
    unit = rs.ROW_UNIT if c.rows > 1 and why != "shape" else 1
    cuts = sorted(int(v) * unit for v in rng.integers(0, c.width // unit + 1, int(rng.integers(0, 5))))
    widths = [b - a for a, b in zip([0] + cuts, cuts + [c.width])]
    hist = rs.hostile_history(rng, c.rows, H) if rng.integers(0, 3) else None
    hi_lead, ho_lead = (int(v) for v in rng.choice([0, 4, 8, 12] + ([2, 6] if why == "align" else []), 2))
    one = rs.want_block(x, hist, hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage)
    ys, at, h, phase = [], 0, hist, c.phase
    for w in widths:
        xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
        ref = rs.want_block(xb, h, hq, c.up, c.decim, phase, c.frac, c.acc, c.stage)
        route, _ = _check(xb, h, taps, c.up, c.decim, phase, c.frac, c.acc, c.stage, ref=ref, x_lead=c.x_lead, y_lead=c.y_lead,
                          hi_lead=hi_lead, ho_lead=ho_lead, what=(why, c, widths, at))
        if ref[0].size and why != "shape":
            assert (route == rs.FAST) == (why == ""), (why, c, widths, at, route)
        ys.append(ref[0])
        at, h, phase = at + w, ref[1], ref[2]
    _same(np.concatenate(ys, axis=1), one[0], (why, c, widths, "chained y"))
    _same(h if h is not None else np.zeros_like(one[1]), one[1], (why, c, widths, "chained hist"))
    assert phase == one[2]


# ---- 9. the host-array entry -------------------------------------------------------------------------
def test_host_entry_agrees_with_the_reference_and_carries_a_stream():
    """fir_cplx_rstream_block through the NumPy entry: two inputs up, two outputs back.  Its device
    buffers come from hipMalloc (x 16-byte aligned, the second array of each pair 256 bytes on), so
    the route is the prediction for aligned addresses."""
    rng = np.random.default_rng(900)
    A = 1 << 30
    for rows, widths, L, U, D, phase, frac, acc, stage in ((3, (516, 0, 8, 260), 72, 3, 2, 1, 12, 32, I32),
                                                           (1, (1001, 1, 300), 128, 16, 15, 14, 12, 24, I32),
                                                           (2, (130, 5, 60), 9, 2, 3, 0, 6, 32, U8),
                                                           (2, (60, 77), 70, 5, 4, 3, 20, 40, I32),
                                                           (2, (100, 0, 31), 3, 4, 3, 2, 12, 32, I32)):
        x = rs.frames(rng, rows, sum(widths))
        hq = rs.taps(rng, L, -40, 41) if stage == U8 else rs.taps(rng, L)
        H = rs.hist_frames(L, U)
        for hist0 in (None, rs.hostile_history(rng, rows, H)):
            one = rs.want_block(x, hist0, hq, U, D, phase, frac, acc, stage)
            ys, at, h, p = [], 0, hist0, phase
            for w in widths:
                xb = x[:, 2 * at:2 * (at + w)]
                y, h, p_next = fir_hip.fir1d_fixed_rows_cplx_resample_block(xb, h, hq, U, D, p, frac, acc, stage)
                ha = 0 if (at == 0 and hist0 is None) or H == 0 else A
                want = rs.predicted_route(A, ha, A, A if H else 0, rows, w, hq, U, D, p, frac, acc, stage)
                assert tuple(crstream.last_launch()) == want, (rows, w, L, U, D, p)
                assert p_next == rs.next_phase(w, U, D, p)
                ys.append(y)
                at, p = at + w, p_next
            _same(np.concatenate(ys, axis=1), one[0], ("host y", rows, widths, L, U, D))
            _same(h, one[1], ("host hist_out", rows, widths, L, U, D))
            assert p == one[2]
    # leading axes, and a block that writes only the history
    x, hq = rs.frames(rng, 6, 40).reshape(2, 3, 80), rs.taps(rng, 9)
    hist = rs.hostile_history(rng, 6, 4).reshape(2, 3, 8)
    y, h, p = crstream.fir1d_fixed_rows_cplx_resample_block(x, hist, hq, 2, 3, 2)
    wy, wh, wp = rs.want_block(x.reshape(6, 80), hist.reshape(6, 8), hq, 2, 3, 2)
    _same(y.reshape(6, -1), wy, "host, leading axes")
    _same(h.reshape(6, -1), wh, "host, leading axes, hist")
    assert p == wp and y.shape[:2] == (2, 3) and h.shape == (2, 3, 8)
    y, h, p = crstream.fir1d_fixed_rows_cplx_resample_block(x[..., :4], hist, hq, 2, 16, 9)
    assert y.shape == (2, 3, 0) and p == 5 == rs.next_phase(2, 2, 16, 9) and tuple(crstream.last_launch()) == (rs.NONE, 0)
    _same(h.reshape(6, -1), rs.want_block(x.reshape(6, 80)[:, :4], hist.reshape(6, 8), hq, 2, 16, 9)[1], "host, history only")
