"""GPU: the four extension libraries (libfir_cdecim.so, libfir_cinterp.so, libfir_cresample.so,
libfir_cstream.so) in one process, beside libfir_hip.so.  They are built over one header-only host
layer (csrc_cext/) and must share none of its state: a launch by one library is recorded by that
library alone.  One tiny call each (1 row of 8 frames, 3 taps, D = 2, U = 3), the values held against
the host references of tests/c*_cases.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cdecim_cases as dc
import cinterp_cases as ic
import cresample_cases as cc
import cstream_cases as sc
from fir_hip import (cdecim, cinterp, cresample, cstream, torch_cdecim, torch_cinterp, torch_cresample, torch_cplx,
                     torch_cstream)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D, U = 2, 3
MODS = {"cdecim": cdecim, "cinterp": cinterp, "cresample": cresample, "cstream": cstream}


def test_a_launch_is_recorded_by_its_own_library_alone():
    rng = np.random.default_rng(20261021)
    x = dc.frames(rng, 1, 8)
    hq = dc.taps(rng, 3)
    hist = sc.hostile_history(rng, 1, 2)
    xd, hd = torch.from_numpy(x).to(DEV), torch.from_numpy(hist).to(DEV)
    hod = torch.empty_like(hd)
    want_y, want_h, _ = sc.want_block(x, hist, hq, D, 1)

    def stream_block(xd, hq, D, phase, out):
        return torch_cstream.fir1d_fixed_rows_cplx_decim_block_dev(xd, hd, hod, hq, D, phase, out=out)

    calls = {
        "cdecim": (torch_cdecim.fir1d_fixed_rows_cplx_decim_dev, (D, 0), dc.want(x, hq, D, 0)),
        "cstream": (stream_block, (D, 1), want_y),
        "cinterp": (torch_cinterp.fir1d_fixed_rows_cplx_interp_dev, (U,), ic.want(x, hq, U)),
        "cresample": (torch_cresample.fir1d_fixed_rows_cplx_resample_dev, (U, D, 0), cc.want(x, hq, U, D, 0)),
    }
    for rnd in range(2):  # twice: the second round starts from records of every library's making
        for name, (entry, rates, want) in calls.items():
            others = {o: MODS[o].last_launch() for o in MODS if o != name}
            yd = torch.empty(want.shape, dtype=torch.int32, device=DEV)
            assert entry(xd, hq, *rates, out=yd) is yd
            launched = MODS[name].last_launch()
            if name == "cstream":
                query = cstream.route(xd.data_ptr(), hd.data_ptr(), yd.data_ptr(), hod.data_ptr(), 1, 8, hq, *rates)
            else:
                query = MODS[name].route(xd.data_ptr(), yd.data_ptr(), 1, 8, hq, *rates)
            assert launched == query and launched.route != MODS[name].ROUTE_NONE, (name, rnd)
            assert {o: MODS[o].last_launch() for o in others} == others, (name, rnd)
            torch.cuda.synchronize()
            got = yd.cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, got, want)
    assert np.array_equal(hod.cpu().numpy(), want_h)
    # the first library's launch leaves all four records alone
    before = {o: MODS[o].last_launch() for o in MODS}
    torch_cplx.fir1d_fixed_rows_cplx_dev(xd, hq)
    torch.cuda.synchronize()
    assert {o: MODS[o].last_launch() for o in MODS} == before
