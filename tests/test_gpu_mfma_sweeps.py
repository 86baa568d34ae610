"""GPU: the steady state of the three persistent 1-D matrix-core kernels (csrc/fir1d_mfma.hip:
fir1d_mfma_step_kernel, fir1d_mfma_run_kernel, fir1d_mfma_long_kernel) against the C oracle.

The other files launch these kernels with at most one or two work units per wave, so whatever
happens between one iteration of a wave and the next -- the step kernel's prefetch of the next
window and its exact vmcnt wait, the run kernel's ring of LDS-DMA buffers, its counted waits, its
row / column cursor and its run-by-run accumulators, the chunked kernel's reuse of its LDS planes
-- ran unchecked.  Here every launch has REQUIRED + 1/2 sweeps of the capped grid (tests/
mfma_sweep_cases.py: the shapes, the pooled images whose reference costs K = 127 rows of oracle
whatever the row count, the restated geometry), and each case asserts, from the launch it recorded:

1. exactly one launch, of the expected kernel and template arguments;
2. every wave did at least REQUIRED[kernel] iterations (from the recorded grid, not the restatement);
3. the share of tile pairs a stale window would get right stays within STALE_CAP;
4. the output equals the reference bit for bit (expanded and compared on the device); a mismatch
   names the first differing (row, col), its tile, and the tile's iteration within its wave (counted
   from 1), so a steady-state bug reads "iteration >= 2 only";
5. no byte outside the output changed (tests/guarded.py; x sits between hostile samples).

No case provokes a fault: every buffer a kernel can touch is backed by the guard allocation.

Durations (MI355X, one pytest --durations=0 run with tests/test_gpu_long_taps.py): the slowest
three cases here 0.52 s (u8-u8-L20-narrow-fast, the first: it loads the library and the pools),
0.15 s (u8-u8-L64-flat-fast) and 0.12 s (u8-u8-L66-flat-fast), every other under 0.1 s, all 144 in
about 8 s; the yardstick, the slowest case of test_gpu_long_taps.py, 20.19 s
(test_table_survives_its_stream_destroyed_mid_launch; its slowest kernel-against-oracle case,
test_int16_2p24_long_filter_vs_c_oracle[1000], 0.87 s).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import fir_hip
import mfma_sweep_cases as mc
from fir_hip import torch_ops
from guarded import guarded_input, guarded_output

DEV = torch.device("cuda:0")
OUT_DTYPE = {mc.U8: torch.uint8, mc.I32: torch.int32}


@functools.lru_cache(maxsize=None)
def _pool_dev(dtype: str, shape: str) -> torch.Tensor:
    return torch.from_numpy(mc.pool_of(dtype, shape)).to(DEV)


@functools.lru_cache(maxsize=None)
def _canon(dtype: str, shape: str) -> np.ndarray:
    return mc.canonical(mc.pool_of(dtype, shape))


def _mismatch(c, g, launch, got: torch.Tensor, want: torch.Tensor) -> str:
    ne = (got != want).reshape(-1)
    first = int(ne.to(torch.uint8).argmax())
    row, col = divmod(first, g.rowlen)
    tile, unit = mc.unit_of(c, g, row, col)
    waves = launch.grid[0] * mc.WG_WAVES
    sweep = mc.first_sweep_outputs(c, g, waves)  # the outputs of every wave's first iteration: a prefix
    return (f"{c.id}: {int(ne.sum())} of {ne.numel()} outputs differ, {int(ne[:sweep].sum())} of them among the {sweep} of "
            f"the waves' first iterations; the first at (row {row}, col {col}): got {int(got.reshape(-1)[first])}, want "
            f"{int(want.reshape(-1)[first])}; tile {tile}, unit {unit}: iteration {unit // waves + 1} of wave {unit % waves}"
            f"{' (iteration >= 2 only)' if unit >= waves else ''}; {launch.inst}")


def _run(c: mc.Case):
    g = mc.geometry(c)
    frac, acc, _ = mc.MODES[c.mode]
    hq = np.asarray(mc.taps(c))
    if c.shape == "flat":
        x = mc.flat_signal(c, g.rowlen)
        xd = guarded_input(torch.from_numpy(x), device=DEV)
        want = torch.from_numpy(mc.reference(c, x)).to(DEV)
        canon_idx = np.zeros(1, np.int64)
    else:
        idx = mc.image_index(c, g.rows)
        idx_dev = torch.from_numpy(idx).to(DEV)
        xd = guarded_input(_pool_dev(c.dtype, c.shape)[idx_dev])
        want = torch.from_numpy(mc.reference(c, mc.pool_of(c.dtype, c.shape))).to(DEV)[idx_dev]
        canon_idx = _canon(c.dtype, c.shape)[idx]
    assert xd.shape == (g.rows, g.rowlen) and xd.data_ptr() % 16 == 0
    yd, guards = guarded_output((g.rows, g.rowlen), OUT_DTYPE[c.stage], device=DEV)
    with fir_hip.launch_log() as log:
        torch_ops.fir1d_fixed_rows_dev(xd, hq, frac, acc, c.stage, out=yd)
    torch.cuda.synchronize()
    # 1. the launch
    assert len(log) == 1, (c.id, [l.inst for l in log])
    launch = log[0]
    name, targs, mode = mc.expected_launch(c)
    if c.kernel == "run":
        assert mc._run_launch(log, c.L, c.stage, c.id) is launch
    assert launch.kernel == name and launch.targs[:len(targs)] == targs, (c.id, launch.inst, name, targs)
    if mode is not None:
        assert launch.note["mode"] == mode, (c.id, launch.note)
    # 2. every wave reached the steady state, and some did one iteration more
    fewest, most = mc.iterations(launch, g.units)
    print(f"{c.id}: {launch.inst} grid {launch.grid[0]}, {g.units} units, {fewest}..{most} iterations per wave", end="")
    assert fewest >= mc.REQUIRED[c.kernel] and most > fewest, (c.id, launch.grid, g.units, fewest, most)
    # 3. a stale window would show
    share = mc.stale_share(canon_idx, g.tiles_per_row, c.tps, launch.grid[0] * mc.WG_WAVES, c.kernel == "step")
    print(f", stale share {share:.4f}")
    assert share <= mc.STALE_CAP, (c.id, share)
    # 4. the result
    if not torch.equal(yd, want):
        raise AssertionError(_mismatch(c, g, launch, yd, want))
    # 5. nothing outside it
    guards(c.id)


@pytest.mark.parametrize("c", mc.STEP_CASES, ids=lambda c: c.id)
def test_step_kernel_past_one_sweep(c):
    _run(c)


@pytest.mark.parametrize("c", mc.RUN_CASES, ids=lambda c: c.id)
def test_run_kernel_past_one_sweep(c):
    _run(c)


@pytest.mark.parametrize("c", mc.LONG_CASES, ids=lambda c: c.id)
def test_long_kernel_past_one_sweep(c):
    _run(c)
