"""GPU: the shared route predicates of the four complex-rate FIR libraries at their thresholds
(csrc_cext/cext_launch.h's needs_wide and dot2_ok, compiled into libfir_cdecim.so, libfir_cinterp.so,
libfir_cresample.so and libfir_cstream.so separately); cases and references: tests/cext_threshold_cases.py,
held to what they claim without a GPU by tests/test_cext_threshold_cases.py.

* needs_wide: 2^16 + 1 complex taps with sum (|hr| + |hi|) = 2^48 - 1 (GENERIC64) and 2^48 (GENERIC128)
  over rows (the stream: a history too) of -32768 samples, so that the generic kernels'
  ``(Acc)(SAcc)(hr * ar) - (Acc)(SAcc)(hi * ai)`` sums reach exactly 2^63 - 32768 and 2^63, in the real
  part in one variant and in the imaginary part in the other.  About 1024 outputs a case are compared
  with the staged exact Python-int sums at (frac, acc, stage) = (12, 64, U8), (12, 65, U8), (40, 65, I32)
  and (40, 100, I32); on the accept side the committed C oracle (the libraries' usual reference) is
  asked as well, for three short runs of them (tests/cext_threshold_cases.py says why not for all).
* dot2_ok: the four neighbours of its limits (+32767 | +32768, -32767 | -32768, acc 32 | 33, frac 31 | 32)
  on rows the fast route takes and on rows only the generic one does, each side bit for bit against the
  library's own reference (``want`` / ``want_block``), over runs of +-32767 / -32768.

Every call asserts predicted_route == the library's route query == last_launch, and that value is the
route the case was built for.  x, y and the stream's histories sit between guards (tests/guarded.py).
No test here provokes a fault: every buffer is in bounds and every size is one the entries accept.

Measured on an MI355X: all 20 tests pass; the module alone takes 20 s, nearly all of it the exact
sums on the host (about 1 s a case) and the C oracle's three runs (accept side): the slowest cases
are cresample-*-accept at 2.2 s, the other accept cases 1.2 to 1.6 s, the reject cases 0.6 s, the
dot2_ok tests 0.01 s each.  Mutation, run once in a scratch copy: with needs_wide's ``>=`` made ``>``
the eight accept cases pass and the eight reject cases fail -- the library takes GENERIC64 where
the rule says GENERIC128 at every acc_bits, and from acc_bits 65 the values are wrong: at (12, 65, U8)
the outputs at 2^63 give 0 for 255, at (40, 65, I32) and (40, 100, I32) -8388608 for 8388608 (355 to
986 of the 2048 compared values, by library); at acc_bits 64 the reference wraps 2^63 to -2^63
itself and only the route differs.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import big_index_cases as bic
import cext_threshold_cases as tc
from fir_hip import torch_cdecim, torch_cinterp, torch_cplx, torch_cresample, torch_cstream
from guarded import guarded_input, guarded_output

DEV = torch.device("cuda:0")
ROUTE = bic.ROUTES


def _entry(lib, xd, hd, hod, yd, taps, frac, acc, stage):
    a = tc.rate_args(lib)
    if lib == "cdecim":
        return torch_cdecim.fir1d_fixed_rows_cplx_decim_dev(xd, taps, *a, frac, acc, stage, out=yd)
    if lib == "cinterp":
        return torch_cinterp.fir1d_fixed_rows_cplx_interp_dev(xd, taps, *a, frac, acc, stage, out=yd)
    if lib == "cresample":
        return torch_cresample.fir1d_fixed_rows_cplx_resample_dev(xd, taps, *a, frac, acc, stage, out=yd)
    return torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(xd, hd, hod, taps, *a, frac, acc, stage, out=yd)


def _run(lib, x, hist, taps, frac, acc, stage, route):
    """One call on guarded buffers.  Returns (y, hist_out or None, findings): findings names every
    disagreement among the route the case was built for, predicted_route, the library's route query
    and last_launch (values are the caller's to compare, so that a wrong route shows its values too)."""
    ext = bic.CEXT[lib][0]
    rows, width = x.shape[0], x.shape[1] // 2
    ow = ext.out_width(width, *tc.rate_args(lib))
    xd = guarded_input(torch.from_numpy(x), device=DEV)
    yd, y_guards = guarded_output((rows, 2 * ow), torch.int32 if stage == tc.I32 else torch.uint8, device=DEV)
    hd = hod = h_guards = None
    if lib == "cstream":
        hd = guarded_input(torch.from_numpy(hist), device=DEV)
        hod, h_guards = guarded_output(hist.shape, torch.int16, device=DEV)
    addrs = tc.addrs_of(lib, xd.data_ptr(), yd.data_ptr(), *((hd.data_ptr(), hod.data_ptr()) if hd is not None else ()))
    pred = tc.predicted(lib, addrs, rows, width, taps.h, frac, acc, stage)
    asked = tuple(ext.route(*addrs, rows, width, taps.h, *tc.rate_args(lib), frac, acc, stage))
    out = _entry(lib, xd, hd, hod, yd, taps, frac, acc, stage)
    launched = tuple(ext.last_launch())
    torch.cuda.synchronize()
    assert out is yd
    y_guards(f"{lib} y")
    if h_guards is not None:
        h_guards(f"{lib} hist_out")
    findings = [f"{what} is {ROUTE[r[0]]}/{r[1]}, not {ROUTE[route]}" for what, r in
                (("predicted_route", pred), ("the route query", asked), ("last_launch", launched)) if r[0] != route]
    if not pred == asked == launched:
        findings.append(f"predicted {pred}, route query {asked}, last_launch {launched}")
    return yd.cpu().numpy(), None if hod is None else hod.cpu().numpy(), findings


# ---- needs_wide ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib,variant,side", tc.wide_ids(), ids=["-".join(i) for i in tc.wide_ids()])
def test_needs_wide_threshold(lib, variant, side):
    w = tc.wide_case(lib, variant, side)
    part = 0 if variant == "re" else 1
    assert int(w.pure.sum()) >= 256 and all(w.sums[j][part] == w.target for j in np.flatnonzero(w.pure))
    taps = torch_cplx.CplxTaps(w.hq)
    findings = []
    for frac, acc, stage in tc.WIDE_STAGES:
        y, hist_out, bad = _run(lib, w.x, w.hist, taps, frac, acc, stage, w.route)
        got = y.reshape(-1, 2)[w.outputs]
        want = tc.staged(w.sums, frac, acc, stage)
        here = [f"route: {b}" for b in bad]
        diff = np.argwhere(got != want)
        if len(diff):
            j, p = (int(v) for v in diff[0])
            here.append(f"{len(diff)} of {want.size} values differ; the first at kept output {int(w.outputs[j])} "
                        f"({'im' if p else 're'}): got {int(got[j, p])}, want {int(want[j, p])}, exact sum {w.sums[j][p]} "
                        f"(2^63 = {1 << 63})")
        if side == "accept":  # |sum| < 2^63: the C oracle's 64-bit sums are exact there too
            at, ref = tc.oracle_spots(w, frac, acc, stage)
            if not np.array_equal(want[at], ref) or not np.array_equal(got[at], ref):
                here.append(f"the C oracle differs at {int((got[at] != ref).sum())} of {ref.size} values from the device, at "
                            f"{int((want[at] != ref).sum())} from the exact sums")
        if hist_out is not None and not np.array_equal(hist_out, np.concatenate([w.hist, w.x], axis=1)[:, -w.hist.shape[1]:]):
            here.append("hist_out is not the last taps - 1 frames of hist_in ++ x")
        findings += [f"[frac {frac}, acc {acc}, stage {'U8' if stage == tc.U8 else 'I32'}] {f}" for f in here]
    assert not findings, f"needs_wide {w.name}: " + "; ".join(findings)


# ---- dot2_ok -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", tc.LIBS)
def test_dot2_ok_neighbours(lib):
    rng = np.random.default_rng(20 + tc.LIBS.index(lib))
    for (rows, width), on in zip(tc.DOT2_SHAPES, (tc.FAST, tc.GENERIC32)):
        x = tc.runs(rng, rows, width)
        hist = bic.cstream_cases.hostile_history(rng, rows, tc.DOT2_TAPS - 1) if lib == "cstream" else None
        for name, stay, fall in tc.dot2_pairs(rng):
            for (hq, frac, acc), route in ((stay, on), (fall, tc.GENERIC64)):
                want_y, want_h = tc.reference(lib, x, hist, hq, frac, acc, tc.I32)
                y, hist_out, bad = _run(lib, x, hist, torch_cplx.CplxTaps(hq), frac, acc, tc.I32, route)
                what = (lib, name, rows, width, frac, acc, ROUTE[route])
                assert not bad, (what, bad)
                assert y.shape == want_y.shape and y.dtype == want_y.dtype, what
                if not np.array_equal(y, want_y):
                    at = np.argwhere(y != want_y)
                    raise AssertionError(f"{what}: {len(at)} of {y.size} values differ; the first at {tuple(int(v) for v in at[0])}: "
                                         f"{y[tuple(at[0])]} != {want_y[tuple(at[0])]}")
                assert want_h is None or np.array_equal(hist_out, want_h), (what, "hist_out")
