"""The argument contract of fir_hip.torch_cplx (tests/torch_cplx_cases.py), run without a GPU.

Every case runs with stand-in tensors (CPU memory, reporting cuda:0 / cuda:1), an explicit ``out=``
and an explicit stream stand-in, against a stub library that records calls and launches nothing: a
refused case must raise FirHipError with the table's text before any library call, an accepted one
must reach exactly ``fir_cplx_rows_dev`` with the expected arguments.  tests/test_gpu_cplx.py runs the
same table on real device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fir_hip
import torch_cplx_cases as cc
import torch_ops_cases as tc
from fir_hip import torch_cplx, torch_ops, torch_resample


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_case(case, monkeypatch):
    cc.run(case, cc.Maker(standin=True), torch_cplx, monkeypatch)


def test_table_covers_the_module_and_leaves_torch_ops_alone():
    """The public callables defined in torch_cplx are the table's entry and the taps holder it
    accepts; nothing of this table is in the torch_ops table, whose entries stay those of torch_ops."""
    public = {n for n, v in vars(torch_cplx).items()
              if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == torch_cplx.__name__}
    assert public == {cc.ENTRY, "CplxTaps"} == set(torch_cplx.__all__)
    assert not hasattr(torch_ops, cc.ENTRY) and not hasattr(torch_resample, cc.ENTRY)
    assert all(c.entry == cc.ENTRY for c in cc.CASES) and not any(c.entry == cc.ENTRY for c in tc.CASES)
    ids = [c.id for c in cc.CASES]
    assert len(set(ids)) == len(ids) and sum(i.endswith("-valid") for i in ids) == 3
    assert all(c.check for c in cc.CASES if c.error is not None)


def test_uses_the_package_loader_and_the_torch_ops_helpers():
    """torch_cplx.lib is the package's loader (what the stub replaces), the checks are torch_ops' own
    helper objects, not copies, and the taps go through the host layer's own (taps, 2) check."""
    assert torch_cplx.lib is fir_hip.lib
    assert torch_cplx._taps_cplx_i32 is fir_hip._taps_cplx_i32
    for name in ("_check_dev", "_rows_of", "_out_dtype", "_check_out", "_no_overlap", "_stream_ptr"):
        assert getattr(torch_cplx, name) is getattr(torch_ops, name), name


def test_stub_reads_the_new_entry_taps():
    stub = cc.StubLib()
    h = np.array([[7, -8], [9, 10], [-11, 12]], np.int32)
    rv = stub.fir_cplx_rows_dev(ctypes.c_void_p(4096), 2, 5, h.ctypes.data_as(ctypes.c_void_p), 3, 12, 32, 1,
                                ctypes.c_void_p(8192), ctypes.c_void_p(0))
    assert rv == 0 and stub.calls == [("fir_cplx_rows_dev", [4096, 2, 5, (7, -8, 9, 10, -11, 12), 3, 12, 32, 1, 8192, 0])]


def test_held_taps_are_converted_once():
    t = torch_cplx.CplxTaps([[1, -2], [3, 4]])
    assert t.n == 2 and t.h.dtype == np.int32 and t.h.shape == (2, 2) and t.h.flags.c_contiguous
    assert t.ptr.value == t.h.ctypes.data
    with pytest.raises(fir_hip.FirHipError, match=r"non-empty \(taps, 2\) array"):
        torch_cplx.CplxTaps([1, 2])


def test_default_arguments():
    """frac_bits 12, acc_bits 32, OUT_I32; no channels argument (a frame is always (re, im))."""
    import inspect

    sig = inspect.signature(torch_cplx.fir1d_fixed_rows_cplx_dev)
    assert list(sig.parameters) == ["x", "hq", "frac_bits", "acc_bits", "out_stage", "out", "stream"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(frac_bits=12, acc_bits=32, out_stage=fir_hip.OUT_I32, out=None, stream=None)
