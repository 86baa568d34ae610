"""The argument contract of fir_hip.torch_resample (tests/torch_resample_cases.py), run without a GPU.

Every case runs with stand-in tensors (CPU memory, reporting cuda:0 / cuda:1), an explicit ``out=``
and an explicit stream stand-in, against a stub library that records calls and launches nothing: a
refused case must raise FirHipError with the table's text before any library call, an accepted one
must reach exactly ``fir_resample_rows_dev`` with the expected arguments.  tests/test_gpu_resample.py
runs the same table on real device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip
import torch_ops_cases as tc
import torch_resample_cases as rc
from fir_hip import torch_interp, torch_ops, torch_resample


@pytest.mark.parametrize("case", rc.CASES, ids=[c.id for c in rc.CASES])
def test_case(case, monkeypatch):
    rc.run(case, rc.Maker(standin=True), torch_resample, monkeypatch)


def test_table_covers_the_module_and_leaves_torch_ops_alone():
    """The one public callable defined in torch_resample is the table's entry; nothing of this
    table is in the torch_ops table, whose entries stay those of torch_ops."""
    public = {n for n, v in vars(torch_resample).items()
              if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == torch_resample.__name__}
    assert public == {rc.ENTRY} == set(torch_resample.__all__)
    assert not hasattr(torch_ops, rc.ENTRY) and not hasattr(torch_interp, rc.ENTRY)
    assert all(c.entry == rc.ENTRY for c in rc.CASES) and not any(c.entry == rc.ENTRY for c in tc.CASES)
    ids = [c.id for c in rc.CASES]
    assert len(set(ids)) == len(ids) and sum(i.endswith("-valid") for i in ids) == 3
    assert all(c.check for c in rc.CASES if c.error is not None)


def test_uses_the_package_loader_and_the_torch_ops_helpers():
    """torch_resample.lib is the package's loader (what the stub replaces), and the checks are
    torch_ops' own helper objects, not copies."""
    assert torch_resample.lib is fir_hip.lib
    assert torch_resample.resample_out_width is fir_hip.resample_out_width
    for name in ("_check_dev", "_taps", "_rows_of", "_out_dtype", "_check_out", "_no_overlap", "_stream_ptr"):
        assert getattr(torch_resample, name) is getattr(torch_ops, name), name


def test_stub_reads_the_new_entry_taps():
    stub = rc.StubLib()
    h = np.array([7, -8, 9], np.int32)
    rv = stub.fir_resample_rows_dev(ctypes.c_void_p(4096), 1, 2, 5, 1, h.ctypes.data_as(ctypes.c_void_p), 3, 4, 3, 2, 12,
                                    32, 1, ctypes.c_void_p(8192), ctypes.c_void_p(0))
    assert rv == 0 and stub.calls == [("fir_resample_rows_dev", [4096, 1, 2, 5, 1, (7, -8, 9), 3, 4, 3, 2, 12, 32, 1, 8192, 0])]


def test_default_arguments():
    """phase 0, frac_bits 12, acc_bits 32, OUT_I32, one channel; out allocated with the resampled shape."""
    import inspect

    sig = inspect.signature(torch_resample.fir1d_fixed_rows_resample_dev)
    assert list(sig.parameters) == ["x", "hq", "up", "decim", "phase", "frac_bits", "acc_bits", "out_stage", "channels",
                                    "out", "stream"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(phase=0, frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, channels=1, out=None,
                            stream=None)
    sig = inspect.signature(fir_hip.fir1d_fixed_rows_resample)
    assert list(sig.parameters) == ["x", "hq", "up", "decim", "phase", "frac_bits", "acc_bits", "out_stage", "channels",
                                    "device", "out"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {k: v.default for k, v in inspect.signature(fir_hip.fir1d_fixed_rows_interp).parameters.items()
                        if v.default is not inspect.Parameter.empty} | dict(phase=0)
