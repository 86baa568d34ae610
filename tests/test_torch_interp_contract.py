"""The argument contract of fir_hip.torch_interp (tests/torch_interp_cases.py), run without a GPU.

Every case runs with stand-in tensors (CPU memory, reporting cuda:0 / cuda:1), an explicit ``out=``
and an explicit stream stand-in, against a stub library that records calls and launches nothing: a
refused case must raise FirHipError with the table's text before any library call, an accepted one
must reach exactly ``fir_interp_rows_dev`` with the expected arguments.  tests/test_gpu_interp.py
runs the same table on real device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip
import torch_interp_cases as ic
import torch_ops_cases as tc
from fir_hip import torch_interp, torch_ops


@pytest.mark.parametrize("case", ic.CASES, ids=[c.id for c in ic.CASES])
def test_case(case, monkeypatch):
    ic.run(case, ic.Maker(standin=True), torch_interp, monkeypatch)


def test_table_covers_the_module_and_leaves_torch_ops_alone():
    """The one public callable defined in torch_interp is the table's entry; nothing of this table
    is in the torch_ops table, whose entries stay those of torch_ops."""
    public = {n for n, v in vars(torch_interp).items()
              if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == torch_interp.__name__}
    assert public == {ic.ENTRY} == set(torch_interp.__all__)
    assert not hasattr(torch_ops, ic.ENTRY)
    assert all(c.entry == ic.ENTRY for c in ic.CASES) and not any(c.entry == ic.ENTRY for c in tc.CASES)
    ids = [c.id for c in ic.CASES]
    assert len(set(ids)) == len(ids) and sum(i.endswith("-valid") for i in ids) == 3
    assert all(c.check for c in ic.CASES if c.error is not None)


def test_uses_the_package_loader_and_the_torch_ops_helpers():
    """torch_interp.lib is the package's loader (what the stub replaces), and the checks are
    torch_ops' own helper objects, not copies."""
    assert torch_interp.lib is fir_hip.lib
    for name in ("_check_dev", "_taps", "_rows_of", "_out_dtype", "_check_out", "_no_overlap", "_stream_ptr"):
        assert getattr(torch_interp, name) is getattr(torch_ops, name), name


def test_stub_reads_the_new_entry_taps():
    stub = ic.StubLib()
    h = np.array([7, -8, 9], np.int32)
    rc = stub.fir_interp_rows_dev(ctypes.c_void_p(4096), 1, 2, 5, 1, h.ctypes.data_as(ctypes.c_void_p), 3, 4, 12, 32, 1,
                                  ctypes.c_void_p(8192), ctypes.c_void_p(0))
    assert rc == 0 and stub.calls == [("fir_interp_rows_dev", [4096, 1, 2, 5, 1, (7, -8, 9), 3, 4, 12, 32, 1, 8192, 0])]


def test_default_arguments():
    """frac_bits 12, acc_bits 32, OUT_I32, one channel; out allocated with the interpolated shape."""
    import inspect

    sig = inspect.signature(torch_interp.fir1d_fixed_rows_interp_dev)
    assert list(sig.parameters) == ["x", "hq", "up", "frac_bits", "acc_bits", "out_stage", "channels", "out", "stream"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, channels=1, out=None, stream=None)
