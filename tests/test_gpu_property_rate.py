"""Property-based GPU parity (hypothesis, derandomized) for the decimating, interpolating, resampling
and complex-tap FIRs: rates, phases, tap counts and values, bit widths, sample types, shapes and
device placement drawn together, each call compared bit for bit with the exact integer references
the fixed grids of test_gpu_decim.py / test_gpu_interp.py / test_gpu_resample.py / test_gpu_cplx.py
already trust (tests/rate_property_cases.py states them once).

Unlike test_gpu_property.py the calls go to the DEVICE entries, with x inside guarded_input and
``out=`` a guarded_output view at drawn leads, so the dispatchers' alignment branches see real
misaligned device pointers and every store outside the output is caught.  Each strategy draws the
route it intends (fast kernel, a generic kernel for one named reason, a forward) and builds a call
that takes it; the test holds ``route_of`` on the real pointers against that route, and the route
OBSERVED in the call's own launch log (``fir_hip.launch_log``: the family's fast kernel, its generic
kernel, or the kernels of the entry it forwards to) against both, so a strategy that stopped
reaching a kernel, or a restated dispatcher that drifted from the library's, fails instead of
passing quietly.  A forwarded call must also equal
the entry it is forwarded to, run on the same guarded x.  A fifth test sends the same cases through
the NumPy host entries with a misaligned host array and ``out=``.

No test here provokes a fault: every buffer a kernel can touch is backed by the guard allocation.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest
import torch
from hypothesis import example, given, settings

import fir_hip
import rate_property_cases as rc
from fir_hip import torch_cplx, torch_interp, torch_ops, torch_resample
from guarded import guarded_input, guarded_output
from test_gpu_property import SETTINGS, _unaligned

DEV = torch.device("cuda:0")
SEEN = {fam: Counter() for fam in rc.FAMILIES}


@pytest.fixture(scope="module", autouse=True)
def _route_shares():
    """After the module: the share of each route among the cases each family's test ran (with -s)."""
    yield
    for fam, seen in SEEN.items():
        n = sum(seen.values())
        if n:
            print(f"\n{fam}: {n} cases, " + ", ".join(f"{r} {seen[r] / n:.3f}" for r in rc.ROUTES[fam]), end="")


def _pinned(fam):
    def deco(f):
        for c in reversed(rc.PINNED[fam]):
            f = example(c)(f)
        return f
    return deco


def _call(c: rc.Case, xd, out):
    """The family's device entry."""
    if c.family == "decim":
        return torch_ops.fir1d_fixed_rows_decim_dev(xd, c.hq, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch, out=out)
    if c.family == "interp":
        return torch_interp.fir1d_fixed_rows_interp_dev(xd, c.hq, c.up, c.frac, c.acc, c.stage, c.ch, out=out)
    if c.family == "resample":
        return torch_resample.fir1d_fixed_rows_resample_dev(xd, c.hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch,
                                                            out=out)
    return torch_cplx.fir1d_fixed_rows_cplx_dev(xd, c.hq, c.frac, c.acc, c.stage, out=out)


def _forwarded(c: rc.Case, xd):
    """What the entry a forward case is handed to gives for the same x."""
    to = rc.forwarded_to(c)
    if to == "decim":
        return torch_ops.fir1d_fixed_rows_decim_dev(xd, c.hq, c.decim, c.phase, c.frac, c.acc, c.stage, c.ch)
    if to == "interp":
        return torch_interp.fir1d_fixed_rows_interp_dev(xd, c.hq, c.up, c.frac, c.acc, c.stage, c.ch)
    return torch_ops.fir1d_fixed_rows_dev(xd, [hr for hr, _ in c.hq], c.frac, c.acc, c.stage, channels=2)


# The kernels of each route, by family; a forward runs the kernels of the entry it is handed to.
FAST_KERNEL = {"decim": "fir1d_decim_kernel", "interp": "fir1d_interp_kernel", "resample": "fir1d_resample_kernel",
               "cplx": "fir1d_cplx_kernel"}
GENERIC_KERNELS = {"decim": {"fir1d_decim_generic_kernel"}, "interp": {"fir1d_interp_generic_kernel"},
                   "resample": {"fir1d_resample_generic_kernel"},
                   "cplx": {"fir1d_cplx_generic_kernel", "fir1d_cplx_generic32_kernel"}}
FORWARD_KERNELS = {"decim": {FAST_KERNEL["decim"]} | GENERIC_KERNELS["decim"],
                   "interp": {FAST_KERNEL["interp"]} | GENERIC_KERNELS["interp"],
                   "rows2": {"fir1d_reg_kernel", "fir1d_generic_kernel", "fir1d_lds_kernel", "fir1d_mfma_step_kernel",
                             "fir1d_mfma_long_kernel"}}


def observed_route(c: rc.Case, log) -> str:
    """The route a call took, read from its launch log: "fast", "generic", "forward", or "none" for a
    call that launched nothing (an empty output)."""
    ks = [l.kernel for l in log]
    if not ks:
        return "none"
    assert len(ks) == 1, (c, [l.inst for l in log])
    if ks[0] == FAST_KERNEL[c.family]:
        return "fast"
    if ks[0] in GENERIC_KERNELS[c.family]:
        return "generic"
    to = rc.forwarded_to(c)
    assert to is not None and ks[0] in FORWARD_KERNELS[to], (c, [l.inst for l in log])
    return "forward"


# Example counts.  The yardstick is test_gpu_property.test_fir1d_rows_random_vs_oracle (1000 examples)
# in the same pytest run: no test here may take longer.  Measured on an MI355X at 400 examples each:
# decim 1.54 s, resample 1.32 s, interp 1.12 s, cplx 0.95 s, the yardstick 2.20 s (nearly all of it is
# drawing the cases).  hypothesis spends about six of seven examples on near-copies of the seventh, so
# the counts below are raised as far as leaves each test a quarter under the yardstick: at 400 / 550
# / 500 / 600 examples decim 1.43 s, interp 1.50 s, resample 1.56 s, cplx 1.53 s, the host entries
# (150) 0.36 s, the yardstick 2.04 s.
def _check(c: rc.Case):
    x = rc.samples(c)
    ref = rc.want(c, x)
    assert ref.shape == (c.rows, rc.out_width(c) * c.ch), c
    xd = guarded_input(torch.from_numpy(x), lead_bytes=c.x_lead, device=DEV)
    yd, guards = guarded_output(ref.shape, torch.int32 if c.stage == rc.I32 else torch.uint8, lead_bytes=c.y_lead, device=DEV)
    assert xd.data_ptr() % 512 == c.x_lead and (ref.size == 0 or yd.data_ptr() % 512 == c.y_lead), c
    assert rc.route_of(c, xd.data_ptr(), yd.data_ptr()) == c.route, c
    SEEN[c.family][c.route] += 1
    with fir_hip.launch_log() as log:
        assert _call(c, xd, yd) is yd
    torch.cuda.synchronize()
    seen = observed_route(c, log)
    assert seen == ("none" if ref.size == 0 else c.route.split(":")[0]), (c, seen, [l.inst for l in log])
    bad = rc.describe_mismatch(c, yd.cpu().numpy(), ref)
    assert bad is None, bad
    guards(f"{c.family} [{c.route}] {c}")
    if c.route == "forward":
        assert torch.equal(yd, _forwarded(c, xd)), f"{c.family} [forward to {rc.forwarded_to(c)}]: differs from that entry; {c}"


@settings(max_examples=400, **SETTINGS)
@_pinned("decim")
@given(rc.decim_case())
def test_decim_random_vs_oracle(case):
    _check(case)


@settings(max_examples=550, **SETTINGS)
@_pinned("interp")
@given(rc.interp_case())
def test_interp_random_vs_oracle(case):
    _check(case)


@settings(max_examples=500, **SETTINGS)
@_pinned("resample")
@given(rc.resample_case())
def test_resample_random_vs_oracle(case):
    _check(case)


@settings(max_examples=600, **SETTINGS)
@_pinned("cplx")
@given(rc.cplx_case())
def test_cplx_random_vs_oracle(case):
    _check(case)


@settings(max_examples=150, **SETTINGS)
@given(rc.any_case())
def test_host_entries_random_vs_oracle(case):
    """The NumPy host entries (fir1d_fixed_rows_decim / _interp / _resample / _cplx) on a misaligned
    host array with out=: they stage x and y in aligned device scratch, so the route is the
    dispatcher's for aligned pointers; the values are the reference's whatever it is."""
    c = case
    x = rc.samples(c)
    ref = rc.want(c, x)
    xin = _unaligned(x, c.x_lead % 7)
    y = _unaligned(np.zeros(ref.shape, ref.dtype), c.y_lead % 5)
    if c.family == "decim":
        got = fir_hip.fir1d_fixed_rows_decim(xin, c.hq, c.decim, c.phase, c.frac, c.acc, c.stage, channels=c.ch, out=y)
    elif c.family == "interp":
        got = fir_hip.fir1d_fixed_rows_interp(xin, c.hq, c.up, c.frac, c.acc, c.stage, channels=c.ch, out=y)
    elif c.family == "resample":
        got = fir_hip.fir1d_fixed_rows_resample(xin, c.hq, c.up, c.decim, c.phase, c.frac, c.acc, c.stage, channels=c.ch, out=y)
    else:
        got = fir_hip.fir1d_fixed_rows_cplx(xin, c.hq, c.frac, c.acc, c.stage, out=y)
    assert got is y
    bad = rc.describe_mismatch(c, got, ref)
    assert bad is None, bad
