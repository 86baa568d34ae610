"""The float64 kernels on NaN, infinities, subnormals and signed zeros (tests/nonfinite_cases.py):
restore (csrc/restore.hip), metrics (metrics.hip), the 1-D ideal model (ideal.hip, ideal_reg.h) and
the 2-D one (ideal2d.hip), each through its host entry and its device-tensor entry, against the
NumPy oracle -- whose outputs tests/test_nonfinite_cases.py ties to the reference's recorded ones.

float64 outputs: equal NaN masks and, elsewhere, equal bit patterns (nonfinite_cases.same_f64);
uint8 outputs: np.array_equal; metrics: conftest.same_metrics.  Every call's kernels are read from
fir_hip.launch_log(), so a case cannot pass on another kernel than the one it was built for.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fir_hip
import nonfinite_cases as nc
from conftest import same_metrics
from fir_hip import torch_ops

DEV = torch.device("cuda:0")


def _ids(cases):
    return [c.id for c in cases]


def _kernels(log):
    return tuple(l.kernel for l in log)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only)


def _off_by_one(a: np.ndarray) -> torch.Tensor:
    """a on the device, one byte past a 16-byte boundary (a slice of a larger uint8 tensor)."""
    assert a.dtype == np.uint8
    big = torch.zeros(a.size + 32, dtype=torch.uint8, device=DEV)
    view = big[1:1 + a.size]
    view.copy_(torch.from_numpy(np.array(a).reshape(-1)))
    assert view.data_ptr() % 16 == 1
    return view.view(a.shape)


# ---- restore -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.cases("restore_u8"), ids=_ids(nc.cases("restore_u8")))
def test_restore(c):
    a, policy, want = c.args["a"], c.args["policy"], nc.expected(c)
    with fir_hip.launch_log() as log:
        got = fir_hip.restore_u8(a, policy)
    assert _kernels(log) == c.kernels
    assert got.dtype == np.uint8 and np.array_equal(got, want), (c.reason, np.flatnonzero(got != want)[:8])
    with fir_hip.launch_log() as log:
        dev = torch_ops.restore_u8_dev(_dev(a), policy)
    assert _kernels(log) == c.kernels
    assert np.array_equal(dev.cpu().numpy(), want), (c.reason, "device-tensor entry")


# csrc/restore.hip: the min/max pass of normalize runs at most kRestoreBlocks workgroups of kBlock
# threads, a thread taking pairs of samples kMinmaxLoads at a time at that grid's stride, then one
# at a time, and thread 0 the odd last sample.  Only an array of more than kMinmaxLoads - 1 strides
# of pairs reaches the first loop, so this is the one size here that is not tiny (21 MB).
MINMAX_STRIDE = 1024 * 256
MINMAX_LOADS = 4


@pytest.fixture(scope="module")
def big_restore_input():
    pairs = (MINMAX_LOADS + 1) * MINMAX_STRIDE + 1000  # one round of the first loop, then one of the second
    a = np.random.default_rng(2623441).uniform(-300.0, 600.0, 2 * pairs + 1)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("where", ["unrolled-loop", "single-loop", "odd-last-sample"])
@pytest.mark.parametrize("kind", ["nan", "extremes"])
def test_restore_normalize_every_loop_of_the_minmax_pass(big_restore_input, where, kind):
    """A NaN, or the array's minimum and maximum, seen only by one of the pass's three loops."""
    a = big_restore_input.copy()
    n = a.size
    idx = {"unrolled-loop": 2 * (2 * MINMAX_STRIDE + 5) + 1,      # load 2 of 4 of thread 5's first round
           "single-loop": 2 * (MINMAX_LOADS * MINMAX_STRIDE + 7),  # thread 7 after the rounds of 4
           "odd-last-sample": n - 1}[where]
    assert n % 2 == 1 and idx < n
    if kind == "nan":
        a[idx] = np.nan
    else:  # both extremes where only that loop reads them (the odd sample: the maximum alone)
        a[idx] = 2000.0
        if where != "odd-last-sample":
            a[idx - 1 if idx % 2 else idx + 1] = -1000.0  # the other half of the same 16-byte load
    want = nc.restore_expected(a, nc.NORMALIZE)
    assert (not want.any()) if kind == "nan" else (want[idx] == 255 and want.any())
    with fir_hip.launch_log() as log:
        dev = torch_ops.restore_u8_dev(_dev(a), nc.NORMALIZE)
    assert _kernels(log) == ("restore_minmax_kernel", "restore_params_kernel", "restore_map_kernel")
    assert log[0].grid == (1024, 1, 1)
    got = dev.cpu().numpy()
    assert np.array_equal(got, want), (where, kind, np.flatnonzero(got != want)[:8])


# ---- metrics -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.cases("compare_metrics"), ids=_ids(nc.cases("compare_metrics")))
def test_metrics(c):
    yi, yf, want = c.args["ideal"], c.args["fixed"], nc.expected(c)
    n = yi.size
    if not c.args["off1"]:  # the host entry copies into fresh (aligned) device buffers
        with fir_hip.launch_log() as log:
            got = fir_hip.compare_metrics(yi, yf)
        assert _kernels(log) == c.kernels
        assert not same_metrics(got, want), (c.reason, {k: (got[k], want[k]) for k in same_metrics(got, want)})
    ideal = _dev(yi)
    fixed = _off_by_one(yf) if c.args["off1"] else _dev(yf)
    assert ideal.data_ptr() % 16 == 0 and (c.args["off1"] or fixed.data_ptr() % 16 == 0)
    out = torch.full((9,), -1.0, dtype=torch.float64, device=DEV)
    work = torch.empty(int(fir_hip.lib().fir_metrics_work_bytes(n)), dtype=torch.uint8, device=DEV)
    with fir_hip.launch_log() as log:
        ret = torch_ops.compare_metrics_dev(ideal, fixed, out=out, work=work)
    assert _kernels(log) == c.kernels
    sums = out.cpu().numpy()
    assert ret is out and sums[8] == 0.0 and sums[7] == n
    got = fir_hip.metrics_from_sums(sums, n)
    assert not same_metrics(got, want), (c.reason, {k: (got[k], want[k]) for k in same_metrics(got, want)})


# ---- ideal, 1-D ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.cases("fir1d_ideal_rows"), ids=_ids(nc.cases("fir1d_ideal_rows")))
def test_ideal_1d(c):
    x, h, want = nc.ideal_x(c.args["shape"]), c.args["h"], nc.expected(c)
    L = len(h)
    with fir_hip.launch_log() as log:
        got = fir_hip.fir1d_ideal_rows(x, h)
    assert _kernels(log) == c.kernels
    assert nc.same_f64(got, want), (c.reason, nc.first_diff(got, want))
    with fir_hip.launch_log() as log:
        dev = torch_ops.fir1d_ideal_rows_dev(_dev(x), h)
    assert _kernels(log) == c.kernels
    assert nc.same_f64(dev.cpu().numpy(), want), (c.reason, "device-tensor entry", nc.first_diff(dev.cpu().numpy(), want))
    # x one byte off the alignment: the generic kernel whatever L is
    with fir_hip.launch_log() as log:
        dev = torch_ops.fir1d_ideal_rows_dev(_off_by_one(x), h)
    assert _kernels(log) == (nc.ideal_kernel(L, True),)
    assert nc.same_f64(dev.cpu().numpy(), want), (c.reason, "x one byte off", nc.first_diff(dev.cpu().numpy(), want))


def test_ideal_images_multi():
    """One fir1d_ideal_images_multi call: two images under the four finite tap sets."""
    xs = [nc.ideal_x(s) for s in nc.IMAGES_MULTI["shapes"]]
    hs = nc.IMAGES_MULTI["hs"]
    got = fir_hip.fir1d_ideal_images_multi(xs, hs)
    specials = 0
    for x, planes in zip(xs, got):
        for h, y in zip(hs, planes):
            want = nc.ideal_expected(x, h)
            specials += int(np.count_nonzero(~np.isfinite(want)))
            assert nc.same_f64(y, want), (x.shape, h, nc.first_diff(y, want))
    assert specials > 0


# ---- ideal, 2-D ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.cases("fir2d_ideal"), ids=_ids(nc.cases("fir2d_ideal")))
def test_ideal_2d(c):
    x, h2, want = nc.ideal2d_x(c.args["shape"]), c.args["h2"], nc.expected(c)
    with fir_hip.launch_log() as log:
        got = fir_hip.fir2d_ideal(x, h2)
    assert _kernels(log) == c.kernels
    assert nc.same_f64(got, want), (c.reason, nc.first_diff(got, want))
    with fir_hip.launch_log() as log:
        dev = torch_ops.fir2d_ideal_dev(_dev(x), h2)
    assert _kernels(log) == c.kernels
    assert nc.same_f64(dev.cpu().numpy(), want), (c.reason, "device-tensor entry", nc.first_diff(dev.cpu().numpy(), want))
