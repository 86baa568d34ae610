"""Property-based GPU parity (hypothesis, derandomized) for the full-rate and 2-D FIRs through their
DEVICE entries: fir1d_fixed_rows_dev, fir1d_fixed_rows_multi_dev, fir1d_fixed_images_multi_dev and
ImagesMultiPlan.launch, fir1d_fixed_segment_dev (and fir1d_fixed_rows_dev + fir1d_fixed_edges_dev on
the same buffers), fir2d_fixed_dev under every FIR2D_PATH, fir1d_ideal_rows_dev and fir2d_ideal_dev.
Tap counts up to 2100, tap values, bit widths, sample types, channels, shapes, halos, image lists
and device placement are drawn together (tests/fullrate_property_cases.py states the strategies,
the dispatchers and the references once), and each call is compared bit for bit with the C oracle
(the 2-D ideal model: tests/ideal2d_ref.py).

Like test_gpu_property_rate.py and unlike test_gpu_property.py (whose host entries stage every call
in aligned scratch), every input sits in guarded_input and every output -- each plane of each image
too -- in a guarded_output view at a drawn byte lead, so the dispatchers' alignment branches see
real device pointers and every store outside an output is caught.  Each strategy draws the route it
intends and builds a call that takes it; a case holds ``route_of`` on the real pointers against that
route, and the kernel names of the call's own launch log (``fir_hip.launch_log``) against
``launches_of``, in order, so a strategy that stopped reaching a kernel, or a restated dispatcher
that drifted from the library's, fails instead of passing quietly.  A segment must also equal its
two-call form, and each plane of an unfused bank the single-filter entry.

No test here provokes a fault: every buffer a kernel can touch is backed by its guard allocation,
and every size is one the entry accepts.

Measured on an MI355X: every test passes and every route of every family runs (the module prints
the shares with -s).  With lds_path_ok's row-length test loosened by one in a local build
(``rowlen % kLdsVec <= 1``; not committed), three tests fail, each on the launch log before any
value is compared: rows [generic:shape] (shrunk to two rows of one u8 sample under 37 taps:
fir1d_lds_kernel<unsigned char, 0, 40, true> where fir1d_generic_kernel was due), bank [each] (two
rows of one sample, 10 taps: the 16-byte-aligned plane of three took fir1d_lds_kernel) and images
[mixed] (a single image of 12 rows of 1041 samples at 8 mod 16 under two zero taps, where the
values cannot differ); segment, fir2d, ideal and the two tall frames pass.
"""
from __future__ import annotations

import os
from collections import Counter

import numpy as np
import pytest
import torch
from hypothesis import example, given, settings

import fir_hip
import fullrate_property_cases as fp
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS

DEV = torch.device("cuda:0")
SEEN = {fam: Counter() for fam in fp.FAMILIES}


@pytest.fixture(scope="module", autouse=True)
def _route_shares():
    """After the module: the share of each route among the cases each family's test ran (with -s)."""
    yield
    for fam, seen in SEEN.items():
        n = sum(seen.values())
        if n:
            print(f"\n{fam}: {n} cases, " + ", ".join(f"{r} {seen[r] / n:.3f}" for r in fp.ROUTES[fam]), end="")


def _pinned(fam):
    def deco(f):
        for c in reversed(fp.pinned_for_hypothesis(fam)):
            f = example(c)(f)
        return f
    return deco


def _out_dtype(c: fp.Case):
    return torch.float64 if c.family == "ideal" else (torch.int32 if c.stage == fp.I32 else torch.uint8)


def _in(a: np.ndarray, lead: int):
    """a inside guarded_input at the lead (an empty tensor has no address to hold to it)."""
    t = guarded_input(torch.from_numpy(a), lead_bytes=lead, device=DEV)
    assert a.size == 0 or t.data_ptr() % 512 == lead
    return t


def _out(shape, c: fp.Case, lead: int):
    t, guards = guarded_output(shape, _out_dtype(c), lead_bytes=lead, device=DEV)
    assert int(np.prod(shape)) == 0 or t.data_ptr() % 512 == lead
    return t, guards


def _same(c: fp.Case, got: torch.Tensor, ref: np.ndarray, what: str = ""):
    bad = fp.describe_mismatch(c, got.cpu().numpy(), ref, what)
    assert bad is None, bad


def _logged(c: fp.Case, log, x_addr, y_addr):
    ks = [l.kernel for l in log]
    assert ks == fp.launches_of(c, x_addr, y_addr), (c, [l.inst for l in log])


def _call(c: fp.Case, xd, yd, halos=(None, None)):
    a = (c.frac, c.acc, c.stage)
    if c.family == "rows":
        return torch_ops.fir1d_fixed_rows_dev(xd, c.hq, *a, c.ch, out=yd)
    if c.family == "bank":
        return torch_ops.fir1d_fixed_rows_multi_dev(xd, c.hq, *a, c.ch, out=yd)
    if c.family == "segment":
        return torch_ops.fir1d_fixed_segment_dev(xd, c.hq, *halos, *a, c.ch, out=yd)
    if c.family == "ideal":
        return (torch_ops.fir1d_ideal_rows_dev if c.route.startswith("1d") else torch_ops.fir2d_ideal_dev)(xd, c.hq, out=yd)
    old = os.environ.pop("FIR2D_PATH", None)
    if c.path is not None:
        os.environ["FIR2D_PATH"] = c.path
    try:
        return torch_ops.fir2d_fixed_dev(xd, c.hq, *a, out=yd)
    finally:
        os.environ.pop("FIR2D_PATH", None)
        if old is not None:
            os.environ["FIR2D_PATH"] = old


# Example counts.  The yardstick is test_gpu_property.test_fir1d_rows_random_vs_oracle (1000 examples)
# in the same pytest run: no test here may take longer.  Measured on an MI355X at 300 examples each:
# rows 1.27 s, bank 1.18 s, segment 0.85 s, fir2d 0.84 s, ideal 0.79 s, the yardstick 2.01 s; images
# took 4.59 s, nearly all of it drawing its image lists value by value and guarding up to 40 planes,
# so an image's sizes and leads now come from one drawn seed and a case holds 16 planes (one in
# twelve: 48).  The counts below are raised as far as leaves each test a quarter under the yardstick:
# at 330 / 440 / 300 / 440 / 580 / 520 examples rows 1.37 s, bank 1.35 s, images 1.49 s, segment
# 1.64 s, fir2d 1.36 s, ideal 1.76 s, the yardstick 2.66 s (another run, in the same order: 1.52, 1.44,
# 1.36, 1.49, 1.51, 1.51 against 2.31).  The two pinned tall frames, timed on their own: 0.07 s
# (gridDim.y = 65535, the register kernel) and 0.03 s (one row more, generic).
def _check(c: fp.Case):
    """rows, bank, segment, fir2d, ideal: one x, one out."""
    x = fp.samples(c)
    ref = fp.want(c, x)
    halos = (None, None)
    if c.family == "segment":
        x, hl, hr = x
        halos = tuple(None if h is None else _in(h, lead) for h, lead in ((hl, c.hl_lead), (hr, c.hr_lead)))
    xd = _in(x, c.x_lead)
    yd, guards = _out(ref.shape, c, c.y_lead)
    xa, ya = xd.data_ptr(), yd.data_ptr()
    assert fp.route_of(c, xa, ya) == c.route, (fp.route_of(c, xa, ya), c)
    SEEN[c.family][c.route] += 1
    with fir_hip.launch_log() as log:
        assert _call(c, xd, yd, halos) is yd
    torch.cuda.synchronize()
    _logged(c, log, xa, ya)
    _same(c, yd, ref)
    guards(f"{c.family} [{c.route}] {c}")
    if c.family == "segment":  # the bulk pass and the edge pass as two calls on the same buffers
        y2, guards2 = _out(ref.shape, c, c.y_lead)
        a = (c.frac, c.acc, c.stage, c.ch)
        torch_ops.fir1d_fixed_rows_dev(xd, c.hq, *a, out=y2)
        assert torch_ops.fir1d_fixed_edges_dev(xd, c.hq, y2, *halos, *a) is y2
        assert torch.equal(y2, yd), f"segment [{c.route}]: rows + edges differs from the one call; {c}"
        guards2(f"segment [{c.route}] rows + edges {c}")
    if c.family == "bank" and c.route == "each":
        for f, h in enumerate(c.hq):
            one = torch_ops.fir1d_fixed_rows_dev(xd, h, c.frac, c.acc, c.stage, c.ch)
            assert torch.equal(yd[f], one), f"bank [each]: plane {f} differs from fir1d_fixed_rows_dev with filter {f}; {c}"


def _check_images(c: fp.Case):
    """fir1d_fixed_images_multi_dev once, then one ImagesMultiPlan launched twice with the inputs
    changed in place between its launches; every plane a guarded_output of its own."""
    x = fp.samples(c)
    ref = fp.want(c, x)
    xs = [_in(xi, im.x_lead) for xi, im in zip(x, c.images)]
    outs, guards = [], []
    for xi, im in zip(x, c.images):
        planes = [_out(xi.shape, c, lead) for lead in im.y_leads]
        outs.append([p for p, _ in planes])
        guards += [g for _, g in planes]
    xa, ya = [t.data_ptr() for t in xs], [[p.data_ptr() for p in ps] for ps in outs]
    assert fp.route_of(c, xa, ya) == c.route, (fp.route_of(c, xa, ya), c)
    SEEN[c.family][c.route] += 1
    a = (c.frac, c.acc, c.stage, c.ch)

    def settle(log, want, what):
        torch.cuda.synchronize()
        _logged(c, log, xa, ya)
        for i, (ps, ri) in enumerate(zip(outs, want)):
            for f, p in enumerate(ps):
                _same(c, p, ri[f], f" {what}, image {i}, plane {f}")

    with fir_hip.launch_log() as log:
        got = torch_ops.fir1d_fixed_images_multi_dev(xs, c.hq, *a, outs=outs)
    assert all(g is o for g, o in zip(got, outs))
    settle(log, ref, "the entry")
    plan = torch_ops.ImagesMultiPlan(xs, c.hq, *a, outs=outs)
    plan.launch()
    x2 = fp.samples(c, again=1)
    for t, xi in zip(xs, x2):  # other samples in the same buffers; the outputs back to the canary
        t.copy_(torch.from_numpy(xi))
    for ps in outs:
        for p in ps:
            p.view(torch.uint8).fill_(0xA5)
    with fir_hip.launch_log() as log:
        plan.launch()
    settle(log, fp.want(c, x2), "the plan's second launch")
    for g in guards:  # once, after all three launches: nothing refills a guard band in between
        g(f"images [{c.route}] {c}")


@settings(max_examples=330, **SETTINGS)
@_pinned("rows")
@given(fp.rows_case())
def test_rows_random_vs_oracle(case):
    _check(case)


@settings(max_examples=440, **SETTINGS)
@_pinned("bank")
@given(fp.bank_case())
def test_bank_random_vs_oracle(case):
    _check(case)


@settings(max_examples=300, **SETTINGS)
@_pinned("images")
@given(fp.images_case())
def test_images_random_vs_oracle(case):
    _check_images(case)


@settings(max_examples=440, **SETTINGS)
@_pinned("segment")
@given(fp.segment_case())
def test_segment_random_vs_oracle(case):
    _check(case)


@settings(max_examples=580, **SETTINGS)
@_pinned("fir2d")
@given(fp.fir2d_case())
def test_fir2d_random_vs_oracle(case):
    _check(case)


@settings(max_examples=520, **SETTINGS)
@_pinned("ideal")
@given(fp.ideal_case())
def test_ideal_random_vs_oracle(case):
    _check(case)


@pytest.mark.parametrize("case", fp.TALL, ids=["gridDim.y=65535", "one_row_more"])
def test_fir2d_tallest_register_frame(case):
    """A 16-pixel-wide frame of 65535 * 16 rows is the largest gridDim.y of the 2-D register kernels;
    one row more and the call takes fir2d_generic_kernel."""
    _check(case)
