"""GPU: the streaming decimating complex-tap FIR with carried history (fir_cplx_stream_block_dev of
libfir_cstream.so, through fir_hip.torch_cstream).

The reference for every value is tests/cstream_cases.py's ``want_block`` (identity 2 of
include/fir_cstream.h over tests/cplx_ref.py's ``want``, the committed C oracle; tests/test_cstream_cases.py
holds it against Python-int loops), so every comparison is np.array_equal, no tolerance: y, hist_out
and next_phase.  Every call asserts that the FIR kernel it launched (last_launch) is what the
library's route query says, and that both are what predicted_route works out from the header's
"Routes" section.  x, hist_in, y and hist_out all sit inside larger allocations between hostile
samples and canaries (tests/guarded.py).  No test here provokes a fault: all buffers are in bounds.

The fast kernel is the decimator's (tests/test_gpu_cdecim.py's docstring has its geometry: tiles of
T = 512 outputs, G = max(1, 16 / D) tiles per workgroup, staging in 16-byte chunks from the boundary
at or below the first window) with a causal window origin, phase - (taps - 1), and a history read
in the staging branch for chunks not wholly inside the block.  So the shapes here are the
decimator's output edges, the block's start (widths below, at and past H, the first chunk across
frame 0 at every lead), and splits of one signal into blocks of one frame, a few frames, up to a
workgroup's input, and multiples of D.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import cdecim_cases as dc
import cstream_cases as sc
import fir_hip
import rate_property_cases as rc
from fir_hip import cstream, torch_cstream
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
I32, U8 = fir_hip.OUT_I32, fir_hip.OUT_U8_SAT
T = sc.T


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} values differ; the first at {tuple(int(v) for v in bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _launch(xd, hd, hod, yd, taps, D, phase, frac, acc, stage, what, route=None, stream=None):
    """One call on device tensors that already sit in guarded buffers: predicted route == the
    library's route query == what was launched.  Returns the prediction."""
    rows = xd.numel() // xd.shape[-1] if xd.shape[-1] else int(np.prod(xd.shape[:-1], dtype=np.int64))
    width = xd.shape[-1] // 2
    addrs = (xd.data_ptr(), 0 if hd is None else hd.data_ptr(), yd.data_ptr(), 0 if hod is None else hod.data_ptr())
    pred = sc.predicted_route(*addrs, rows, width, taps.h, D, phase, frac, acc, stage)
    if route is not None:
        assert pred[0] == route, (what, pred)
    assert tuple(cstream.route(*addrs, rows, width, taps.h, D, phase, frac, acc, stage)) == pred, what
    out = torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(xd, hd, hod, taps, D, phase, frac, acc, stage, out=yd,
                                                              stream=stream)
    assert out is yd
    assert tuple(cstream.last_launch()) == pred, (what, cstream.last_launch(), pred)
    return pred


def _check(x, hist, hq, D, phase=0, frac=12, acc=32, stage=I32, *, route=None, ref=None, x_lead=0, y_lead=0, hi_lead=0,
           ho_lead=0, what=""):
    """One block on guarded buffers against want_block (or ``ref``): y, hist_out, the guards."""
    rows, width = x.shape[0], x.shape[1] // 2
    taps = hq if isinstance(hq, torch_cstream.CplxTaps) else torch_cstream.CplxTaps(hq)
    want_y, want_h, want_p = ref if ref is not None else sc.want_block(x, hist, taps.h, D, phase, frac, acc, stage)
    assert want_y.shape == (rows, 2 * sc.out_width(width, D, phase)), what
    xd = guarded_input(torch.from_numpy(x), lead_bytes=x_lead, device=DEV)
    hd = None if hist is None else guarded_input(torch.from_numpy(hist), lead_bytes=hi_lead, device=DEV)
    yd, y_guards = guarded_output(want_y.shape, torch.int32 if stage == I32 else torch.uint8, lead_bytes=y_lead, device=DEV)
    hod, h_guards = guarded_output(want_h.shape, torch.int16, lead_bytes=ho_lead, device=DEV)
    pred = _launch(xd, hd, hod, yd, taps, D, phase, frac, acc, stage, what, route)
    assert cstream.next_phase(width, D, phase) == want_p == cstream.lib().fir_cplx_stream_next_phase(width, D, phase), what
    torch.cuda.synchronize()
    _same(yd.cpu().numpy(), want_y, (what, "y"))
    if taps.n > 1:
        _same(hod.cpu().numpy(), want_h, (what, "hist_out"))
    y_guards(f"{what} y")
    h_guards(f"{what} hist_out")
    return pred


# ---- 1. one block, zero and hostile history ----------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 5, 33, 64])
def test_one_block_zero_and_hostile_history(L):
    rng = np.random.default_rng(10 + L)
    taps = torch_cstream.CplxTaps(sc.taps(rng, L))
    bucket = min(b for b in sc.BUCKETS if b >= L)
    for D in (2, 3, 16):
        for i, ow in enumerate(dc.edge_out_widths(D)):
            for phase in (0, D - 1):
                width = dc.width_for(ow, D, phase, slack=(D - 1) * (i % 2))
                x = sc.frames(rng, 1, width)
                for hist in (None, sc.hostile_history(rng, 1, L - 1)):
                    got = _check(x, hist, taps, D, phase, what=(L, D, phase, width, hist is None))
                    assert got == (sc.FAST, bucket)


# ---- 2. the row start --------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 5, 33, 64])
def test_the_block_start(L):
    """Widths below, at and past H, so that hist_out mixes hist_in and x; phase >= width (no output,
    the history still written); and the first window's 16-byte chunk across frame 0 at every lead:
    the window of output 0 starts at frame phase - H, so (phase - H) mod 4 takes its four values."""
    rng = np.random.default_rng(20 + L)
    H = L - 1
    taps = torch_cstream.CplxTaps(sc.taps(rng, L))
    bucket = min(b for b in sc.BUCKETS if b >= L)
    leads = set()
    for D in (2, 3, 16):
        for width in sorted({1, 2, 3, max(1, H - 1), H, H + 1, 4, 5, 8}):
            x = sc.frames(rng, 1, width)
            for phase in sorted({0, 1, D - 1}):
                for hist in (None, sc.hostile_history(rng, 1, H)):
                    want = (sc.FAST, bucket) if width > phase else (sc.NONE, 0)
                    assert _check(x, hist, taps, D, phase, what=(L, D, phase, width, hist is None)) == want
    for D, phases in ((4, range(4)), (16, range(16)), (3, range(3))):
        for phase in phases:
            leads.add((phase - H) % 4)
            for width in (phase + 1, 2 * T * D + phase + 3):  # one output; two tiles and some
                x = sc.frames(rng, 1, width)
                for hist in (None, sc.hostile_history(rng, 1, H)):
                    assert _check(x, hist, taps, D, phase, what=("lead", L, D, phase, width)) == (sc.FAST, bucket)
    assert leads == {0, 1, 2, 3}


# ---- 3. split invariance on the device ---------------------------------------------------------------
def _splits(rng, N, D, G):
    return {
        "one-frame blocks": [1] * 200 + [N - 200],
        "widths in [0, 3 D]": sc.random_split(rng, N, 3 * D),
        "up to a workgroup's input": sc.random_split(rng, N, G * T * D),
        "multiples of D": [D * w for w in sc.random_split(rng, N // D, 3 * G * T // 2)] + ([N % D] if N % D else []),
    }


@pytest.mark.parametrize("D", [2, 16])
def test_split_invariance_one_row(D):
    """One row of 2 G T D + 37 D + 1 frames cut four ways; every block reads its frames in place, out
    of ONE guarded copy of the row (its neighbours are the frames before and after it), and writes
    its kept frames in place into one guarded output; the histories ping-pong between two guarded
    buffers.  Compared with the single-block reference, final history and phase included."""
    rng = np.random.default_rng(30 + D)
    G = sc.tiles_per_group(D)
    N = 2 * G * T * D + 37 * D + 1
    L = 33
    H = L - 1
    taps = torch_cstream.CplxTaps(sc.taps(rng, L))
    x, hist0 = sc.frames(rng, 1, N), sc.hostile_history(rng, 1, H)
    for hist in (hist0, None):
        for phase0 in (0, D - 1):
            want_y, want_h, want_p = sc.want_block(x, hist, taps.h, D, phase0)
            assert _check(x, hist, taps, D, phase0, ref=(want_y, want_h, want_p), what=("whole", D)) == (sc.FAST, 48)
            for name, widths in _splits(rng, N, D, G).items():
                assert sum(widths) == N
                xd = guarded_input(torch.from_numpy(x), device=DEV)
                yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
                hb, hg = zip(*(guarded_output((1, 2 * H), torch.int16, device=DEV) for _ in range(2)))
                cur, at, done, phase, routes = None, 0, 0, phase0, set()
                if hist is not None:
                    hb[0].copy_(torch.from_numpy(hist))
                    cur = 0
                for w in widths:
                    ow = sc.out_width(w, D, phase)
                    nxt = 1 if cur is None else 1 - cur
                    routes.add(_launch(xd[:, 2 * at:2 * (at + w)], None if cur is None else hb[cur], hb[nxt],
                                       yd[:, 2 * done:2 * (done + ow)], taps, D, phase, 12, 32, I32, (name, at, w))[0])
                    phase, at, done, cur = cstream.next_phase(w, D, phase), at + w, done + ow, nxt
                torch.cuda.synchronize()
                assert phase == want_p and 2 * done == want_y.shape[1], name
                _same(yd.cpu().numpy(), want_y, (D, name, "y"))
                _same(hb[cur].cpu().numpy(), want_h, (D, name, "hist_out"))
                y_guards(name)
                for g in hg:
                    g(name)
                assert routes <= {sc.FAST, sc.GENERIC32, sc.NONE} and sc.FAST in routes, (name, routes)


@pytest.mark.parametrize("D", [2, 16])
def test_split_invariance_rows(D):
    """5 rows, blocks of a multiple of 4 frames: every block is FAST, each on its own guarded buffers."""
    rng = np.random.default_rng(35 + D)
    G = sc.tiles_per_group(D)
    N = (2 * G * T * D + 37 * D + 1) // 4 * 4
    L, rows = 24, 5
    taps = torch_cstream.CplxTaps(sc.taps(rng, L))
    x, hist = sc.frames(rng, rows, N), sc.hostile_history(rng, rows, L - 1)
    one = sc.want_block(x, hist, taps.h, D, D - 1)
    assert _check(x, hist, taps, D, D - 1, ref=one, what=("whole", D)) == (sc.FAST, 24)
    for name, widths in (("4-frame blocks", [4] * 20 + [N - 80]),
                         ("up to a workgroup's input", [4 * w for w in sc.random_split(rng, N // 4, G * T * D // 4)]),
                         ("multiples of 4 D", [4 * D * w for w in sc.random_split(rng, N // (4 * D), 2 * G * T // 4)] + [N % (4 * D)])):
        ys, at, h, phase = [], 0, hist, D - 1
        for w in widths:
            xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
            ref = sc.want_block(xb, h, taps.h, D, phase)
            got = _check(xb, h, taps, D, phase, ref=ref, what=(D, name, at, w))
            assert got == ((sc.FAST, 24) if ref[0].size else (sc.NONE, 0)), (name, at, w, got)
            ys.append(ref[0])
            at, h, phase = at + w, ref[1], ref[2]
        # the per-block references chain to the single-block one (the device equalled each of them)
        _same(np.concatenate(ys, axis=1), one[0], (D, name, "y"))
        _same(h, one[1], (D, name, "hist_out"))
        assert phase == one[2]


# ---- 4. rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 16])
def test_rows(D):
    rng = np.random.default_rng(40 + D)
    for L in (1, 5, 33, 64):
        taps = torch_cstream.CplxTaps(sc.taps(rng, L))
        for rows, width in dc.multi_row_shapes(D) + [(3, 6), (7, 6)]:
            x = sc.frames(rng, rows, width)
            for phase in (0, D - 1):
                for hist in (None, sc.hostile_history(rng, rows, L - 1)):
                    want = sc.NONE if width <= phase else (sc.FAST if width % 4 == 0 else sc.GENERIC32)
                    _check(x, hist, taps, D, phase, route=want, what=(L, D, phase, rows, width))


# ---- 5. every tap count ------------------------------------------------------------------------------
def test_every_tap_count():
    """Taps 1..64 on one row of two workgroups and some, D = 3, a hostile history: every bucket; the
    reported bucket is the smallest that holds the taps."""
    rng = np.random.default_rng(50)
    D = 3
    G = sc.tiles_per_group(D)
    x = sc.frames(rng, 1, 2 * G * T * D + 37 * D + 1)
    for L in range(1, 65):
        hq = sc.taps(rng, L)
        want = (sc.FAST, min(b for b in sc.BUCKETS if b >= L))
        assert _check(x, sc.hostile_history(rng, 1, L - 1), hq, D, L % D, what=(L, D)) == want


# ---- 6. generic routes -------------------------------------------------------------------------------
def _three_blocks(x, hist, hq, D, phase, widths, frac=12, acc=32, stage=I32, *, route, block=sc.want_block, what="", **leads):
    at, one = 0, block(x, hist, hq, D, phase, frac, acc, stage)
    ys = []
    for w in widths:
        xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
        ref = block(xb, hist, hq, D, phase, frac, acc, stage)
        want = (route if ref[0].size else sc.NONE) if route is not None else None
        _check(xb, hist, hq, D, phase, frac, acc, stage, ref=ref, route=want, what=(what, at, w), **leads)
        ys.append(ref[0])
        at, hist, phase = at + w, ref[1], ref[2]
    assert at == x.shape[1] // 2
    _same(np.concatenate(ys, axis=1), one[0], (what, "chained y"))
    _same(hist, one[1], (what, "chained hist"))
    assert phase == one[2]


def test_generic_routes_across_three_blocks():
    rng = np.random.default_rng(60)
    g32, g64 = sc.GENERIC32, sc.GENERIC64
    for rows, widths in ((1, (700, 3, 1500)), (3, (1028, 40, 260)), (2, (5, 0, 600))):
        N = sum(widths)
        x = sc.frames(rng, rows, N)

        def run(hq, D, phase, *a, route, what, none_too=True, **k):
            h = sc.hostile_history(rng, rows, len(hq) - 1)
            for hist in ((h, None) if none_too else (h,)):
                _three_blocks(x, hist, hq, D, phase, widths, *a, route=route, what=(what, rows, hist is None), **k)

        run(sc.taps(rng, 16), 1, 0, route=g32, what="D = 1")
        run(sc.taps(rng, 16), 17, 5, route=g32, what="D = 17")
        run(sc.taps(rng, 65), 3, 2, route=g32, what="65 taps")
        run(sc.taps(rng, 9, -40, 41), 2, 1, 6, 32, U8, route=g32, what="u8 stage")
        run(sc.taps(rng, 16), 4, 3, route=g32, what="x 4 bytes off 16", x_lead=4)
        h = sc.taps(rng, 9)
        h[3, 0] = 40000
        run(h, 3, 1, route=g64, what="a part of 40000")
        run(sc.taps(rng, 16), 2, 0, 20, 40, route=g64, what="acc 40")
        run(sc.taps(rng, 5), 5, 4, 12, 64, route=g64, what="acc 64")
        run(sc.taps(rng, 7), 3, 0, route=g64, what="x 2 bytes off 4", x_lead=2, none_too=False)
        run(sc.taps(rng, 7), 3, 0, route=g64, what="hist_in 2 bytes off 4", hi_lead=2, none_too=False)
        run(sc.taps(rng, 7), 3, 0, route=g64, what="hist_out 2 bytes off 4", ho_lead=2)
        run(sc.taps(rng, 7), 3, 0, route=None, what="histories 4 off 16", hi_lead=4, ho_lead=12)  # fast where x allows


def test_generic128_across_three_blocks():
    """needs_wide: 2^16 + 9 complex taps of +-(2^31 - 1) make sum(|hr| + |hi|) * 32768 pass 2^63, so the
    kernel sums in 128 bits.  The reference is want_block_kept (Python ints over the kept frames; a
    full-rate loop over a history of 2^16 frames is out of reach), so the blocks are a few frames."""
    rng = np.random.default_rng(63)
    L = (1 << 16) + 9
    hq = np.where(rng.integers(0, 2, (L, 2)) == 0, (1 << 31) - 1, -(1 << 31) + 1).astype(np.int64)
    assert dc.sum_can_pass_2_63(hq)
    x = sc.frames(rng, 2, 12)
    for hist in (sc.hostile_history(rng, 2, L - 1), None):
        for frac, acc, stage in ((30, 64, I32), (40, 80, U8)):
            _three_blocks(x, hist, hq, 3, 1, (5, 1, 6), frac, acc, stage, route=sc.GENERIC128, block=sc.want_block_kept,
                          what=("wide", frac, acc, hist is None))


# ---- 7. hist_out = None; taps = 1 --------------------------------------------------------------------
def test_no_hist_out_writes_nothing_and_one_tap_ignores_both():
    rng = np.random.default_rng(70)
    for L, D, rows, width in ((33, 4, 1, 3000), (5, 3, 3, 1030), (9, 2, 4, 1028)):
        x, hist, hq = sc.frames(rng, rows, width), sc.hostile_history(rng, rows, L - 1), sc.taps(rng, L)
        taps = torch_cstream.CplxTaps(hq)
        want_y, _, _ = sc.want_block(x, hist, hq, D, 1)
        xd, hd = guarded_input(torch.from_numpy(x), device=DEV), guarded_input(torch.from_numpy(hist), device=DEV)
        yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
        dummy, d_guards = guarded_output((rows, 2 * (L - 1)), torch.int16, device=DEV)  # never passed: stays canary
        pred = _launch(xd, hd, None, yd, taps, D, 1, 12, 32, I32, ("no hist_out", L))
        assert pred[0] in (sc.FAST, sc.GENERIC32)
        torch.cuda.synchronize()
        _same(yd.cpu().numpy(), want_y, ("no hist_out", L))
        y_guards("no hist_out y")
        d_guards("no hist_out dummy")
        assert bool((dummy.view(torch.uint8) == 0xA5).all())
    for D, rows, width in ((2, 1, 3001), (16, 4, 1028), (1, 2, 77)):
        x, hq = sc.frames(rng, rows, width), sc.taps(rng, 1)
        want_y, want_h, _ = sc.want_block(x, None, hq, D, D - 1)
        assert want_h.shape == (rows, 0)
        xd = guarded_input(torch.from_numpy(x), device=DEV)
        yd, y_guards = guarded_output(want_y.shape, torch.int32, device=DEV)
        pred = _launch(xd, None, None, yd, torch_cstream.CplxTaps(hq), D, D - 1, 12, 32, I32, ("one tap", D))
        assert pred == ((sc.FAST, 2) if D > 1 else (sc.GENERIC32, 0))
        torch.cuda.synchronize()
        _same(yd.cpu().numpy(), want_y, ("one tap", D))
        y_guards("one tap")
        _check(x, np.zeros((rows, 0), np.int16), hq, D, 0, what=("one tap, empty histories", D))
    # width = 0: the history is copied (zeros for None); rows of no frames
    for rows, L in ((1, 5), (3, 33)):
        hist, hq = sc.hostile_history(rng, rows, L - 1), sc.taps(rng, L)
        for h in (hist, None):
            assert _check(np.zeros((rows, 0), np.int16), h, hq, 3, 2, what=("width 0", rows, L)) == (sc.NONE, 0)


# ---- 8. CplxDecimStream ------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (3,), (2, 2)])
def test_stream_object(lead):
    rng = np.random.default_rng(80 + len(lead))
    L, D = 24, 5
    hq = sc.taps(rng, L)
    rows = int(np.prod(lead, dtype=np.int64))
    widths = [0, 1, 7, 4096, 0, 23, 3, 8192 + 4, 12, 5]
    N = sum(widths)
    x = sc.frames(rng, rows, N)
    s = torch_cstream.CplxDecimStream(hq, D, lead, phase=2, device=DEV)
    assert (s.phase, s.frames_in, s.frames_out) == (2, 0, 0) and s.history.shape == lead + (2 * (L - 1),)
    for rnd, (hist, phase) in enumerate(((None, 2), (sc.hostile_history(rng, rows, L - 1), 4))):
        if rnd:
            s.reset(torch.from_numpy(hist.reshape(lead + (-1,))).to(DEV), phase)
            assert (s.phase, s.frames_in, s.frames_out) == (phase, 0, 0)
        want_y, want_h, want_p = sc.want_block(x, hist, hq, D, phase)
        ys, at = [], 0
        for w in widths:
            xb = guarded_input(torch.from_numpy(np.ascontiguousarray(x[:, 2 * at:2 * (at + w)]).reshape(lead + (2 * w,))), device=DEV)
            ys.append(s.push(xb))
            at += w
            assert s.frames_in == at and s.frames_out == sc.out_width(at, D, phase)
        torch.cuda.synchronize()
        got = torch.cat(ys, dim=-1).cpu().numpy().reshape(rows, -1)
        _same(got, want_y, ("stream", lead, rnd))
        _same(s.history.cpu().numpy().reshape(rows, -1), want_h, ("stream history", lead, rnd))
        assert s.phase == want_p
    s.reset()
    assert (s.phase, s.frames_in, s.frames_out) == (0, 0, 0) and not bool(s.history.any())
    with pytest.raises(fir_hip.FirHipError, match="leading axes"):
        s.push(torch.zeros(lead + (1, 8), dtype=torch.int16, device=DEV))


# ---- 9. graph capture --------------------------------------------------------------------------------
def test_two_blocks_are_captured_once_and_replayed():
    """The fast route allocates nothing and reads no device table: two blocks (history A -> B, then
    B -> A) captured into one graph, a linear chain of four kernels, replayed on fresh block pairs."""
    rng = np.random.default_rng(90)
    rows, D, phase, L = 4, 4, 3, 33
    width = 1028 // D * D
    assert width % D == 0 and width % 4 == 0
    taps = torch_cstream.CplxTaps(sc.taps(rng, L))
    ow = sc.out_width(width, D, phase)
    assert sc.next_phase(width, D, phase) == phase
    side = torch.cuda.Stream(device=DEV)
    xs = guarded_input(torch.zeros((2, rows, 2 * width), dtype=torch.int16), device=DEV)  # static input
    ys, y_guards = guarded_output((2, rows, 2 * ow), torch.int32, device=DEV)
    (ha, ga), (hb, gb) = (guarded_output((rows, 2 * (L - 1)), torch.int16, device=DEV) for _ in range(2))

    def pair(what):
        for k, (hi, ho) in enumerate(((ha, hb), (hb, ha))):
            assert _launch(xs[k], hi, ho, ys[k], taps, D, phase, 12, 32, I32, (what, k), route=sc.FAST, stream=side) == (sc.FAST, 48)

    with torch.cuda.stream(side):
        pair("warm-up")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pair("capture")
    torch.cuda.synchronize()
    hist0 = sc.hostile_history(rng, rows, L - 1)
    blocks = [sc.frames(rng, rows, width) for _ in range(6)]
    want_y, want_h, _ = sc.want_block(np.concatenate(blocks, axis=1), hist0, taps.h, D, phase)
    ha.copy_(torch.from_numpy(hist0))
    got = []
    for rep in range(3):
        xs.copy_(torch.from_numpy(np.stack(blocks[2 * rep:2 * rep + 2])))
        ys.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got += [ys[0].cpu().numpy(), ys[1].cpu().numpy()]
    _same(np.concatenate(got, axis=1), want_y, "replays")
    _same(ha.cpu().numpy(), want_h, "history after the replays")
    # the eager calls give the same
    ha.copy_(torch.from_numpy(hist0))
    eager = []
    for rep in range(3):
        xs.copy_(torch.from_numpy(np.stack(blocks[2 * rep:2 * rep + 2])))
        with torch.cuda.stream(side):
            pair("eager")
        torch.cuda.synchronize()
        eager += [ys[0].cpu().numpy(), ys[1].cpu().numpy()]
    _same(np.concatenate(eager, axis=1), want_y, "eager")
    y_guards("graph y")
    ga("history A")
    gb("history B")


# ---- 10. random cases --------------------------------------------------------------------------------
@settings(max_examples=40, **SETTINGS)
@given(dc.property_case(), st.integers(0, 2**32 - 1))
def test_random_splits_vs_oracle(case, seed):
    """tests/cdecim_cases.property_case (taps, D, phase, rows, width, x and y leads, a reason off the
    fast route for about half the cases) cut into up to 5 blocks, the histories at drawn leads."""
    why, c = case
    rng = np.random.default_rng(seed)
    x = rc.samples(c)
    hq = np.asarray(c.hq, dtype=np.int64)
    taps = torch_cstream.CplxTaps(hq)
    unit = sc.ROW_UNIT if c.rows > 1 and why != "shape" else 1
    cuts = sorted(int(v) * unit for v in rng.integers(0, c.width // unit + 1, int(rng.integers(0, 5))))
    widths = [b - a for a, b in zip([0] + cuts, cuts + [c.width])]
    hist = sc.hostile_history(rng, c.rows, taps.n - 1) if rng.integers(0, 3) else None
    hi_lead, ho_lead = (int(v) for v in rng.choice([0, 4, 8, 12] + ([2, 6] if why == "align" else []), 2))
    one = sc.want_block(x, hist, hq, c.decim, c.phase, c.frac, c.acc, c.stage)
    ys, at, h, phase = [], 0, hist, c.phase
    for w in widths:
        xb = np.ascontiguousarray(x[:, 2 * at:2 * (at + w)])
        ref = sc.want_block(xb, h, hq, c.decim, phase, c.frac, c.acc, c.stage)
        route, _ = _check(xb, h, taps, c.decim, phase, c.frac, c.acc, c.stage, ref=ref, x_lead=c.x_lead, y_lead=c.y_lead,
                          hi_lead=hi_lead, ho_lead=ho_lead, what=(why, c, widths, at))
        if ref[0].size and why != "shape":
            assert (route == sc.FAST) == (why == ""), (why, c, widths, at, route)
        ys.append(ref[0])
        at, h, phase = at + w, ref[1], ref[2]
    _same(np.concatenate(ys, axis=1), one[0], (why, c, widths, "chained y"))
    _same(h if h is not None else np.zeros_like(one[1]), one[1], (why, c, widths, "chained hist"))
    assert phase == one[2]


# ---- 11. the host-array entry ------------------------------------------------------------------------
def test_host_entry_agrees_with_the_reference_and_carries_a_stream():
    """fir_cplx_stream_block through the NumPy entry: two inputs up, two outputs back.  Its device
    buffers come from hipMalloc (x 16-byte aligned, the second array of each pair 256 bytes on), so
    the route is the prediction for aligned addresses."""
    rng = np.random.default_rng(110)
    A = 1 << 30
    for rows, widths, L, D, phase, frac, acc, stage in ((3, (2052, 0, 8, 1028), 33, 3, 1, 12, 32, I32),
                                                        (1, (9001, 1, 3000), 64, 16, 15, 12, 24, I32),
                                                        (2, (1030, 5, 600), 9, 2, 0, 6, 32, U8),
                                                        (2, (600, 77), 70, 5, 4, 20, 40, I32),
                                                        (4, (6, 2, 40), 5, 8, 7, 12, 32, I32),
                                                        (2, (100, 0, 31), 1, 4, 2, 12, 32, I32)):
        x = sc.frames(rng, rows, sum(widths))
        hq = sc.taps(rng, L, -40, 41) if stage == U8 else sc.taps(rng, L)
        for hist0 in (None, sc.hostile_history(rng, rows, L - 1)):
            one = sc.want_block(x, hist0, hq, D, phase, frac, acc, stage)
            ys, at, h, p = [], 0, hist0, phase
            for w in widths:
                xb = x[:, 2 * at:2 * (at + w)]
                y, h, p_next = fir_hip.fir1d_fixed_rows_cplx_decim_block(xb, h, hq, D, p, frac, acc, stage)
                ha = 0 if (at == 0 and hist0 is None) or L == 1 else A
                want = sc.predicted_route(A, ha, A, A if L > 1 else 0, rows, w, hq, D, p, frac, acc, stage)
                assert tuple(cstream.last_launch()) == want, (rows, w, L, D, p)
                assert p_next == sc.next_phase(w, D, p)
                ys.append(y)
                at, p = at + w, p_next
            _same(np.concatenate(ys, axis=1), one[0], ("host y", rows, widths, L, D))
            _same(h, one[1], ("host hist_out", rows, widths, L, D))
            assert p == one[2]
    # leading axes, and a block that writes only the history
    x, hq = sc.frames(rng, 6, 40).reshape(2, 3, 80), sc.taps(rng, 5)
    hist = sc.hostile_history(rng, 6, 4).reshape(2, 3, 8)
    y, h, p = cstream.fir1d_fixed_rows_cplx_decim_block(x, hist, hq, 3, 2)
    wy, wh, wp = sc.want_block(x.reshape(6, 80), hist.reshape(6, 8), hq, 3, 2)
    _same(y.reshape(6, -1), wy, "host, leading axes")
    _same(h.reshape(6, -1), wh, "host, leading axes, hist")
    assert p == wp and y.shape[:2] == (2, 3) and h.shape == (2, 3, 8)
    y, h, p = cstream.fir1d_fixed_rows_cplx_decim_block(x[..., :4], hist, hq, 16, 7)
    assert y.shape == (2, 3, 0) and p == 5 and tuple(cstream.last_launch()) == (sc.NONE, 0)
    _same(h.reshape(6, -1), sc.want_block(x.reshape(6, 80)[:, :4], hist.reshape(6, 8), hq, 16, 7)[1], "host, history only")
