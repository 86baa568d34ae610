"""The argument contract of fir_hip.torch_ops (tests/torch_ops_cases.py), run without a GPU.

Every case runs with stand-in tensors (CPU memory, reporting cuda:0 / cuda:1), an explicit
``out=`` and an explicit stream stand-in, against a stub library that records calls and launches
nothing: a refused case must raise FirHipError with the table's text before any library call, an
accepted one must reach exactly the expected C entry with the expected arguments.
tests/test_gpu_torch_ops_contract.py runs the same table on real device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import fir_hip
import torch_ops_cases as tc
from fir_hip import torch_ops


@pytest.mark.parametrize("case", tc.CASES, ids=[c.id for c in tc.CASES])
def test_case(case, monkeypatch):
    tc.run_case(case, tc.Maker(standin=True), torch_ops, monkeypatch)


def test_table_covers_every_public_entry():
    """Every public callable of torch_ops is in the table (Taps is the taps argument of the others;
    ImagesMultiPlan is what fir1d_fixed_images_multi_dev constructs and launches)."""
    public = {n for n, v in vars(torch_ops).items()
              if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == torch_ops.__name__}
    assert public - {"Taps", "ImagesMultiPlan"} == set(tc.ENTRIES)
    for entry in tc.ENTRIES:
        ids = [c.id for c in tc.CASES if c.entry == entry]
        assert any(i.endswith("-valid") for i in ids) and len(ids) > 2, entry


def test_every_refused_case_names_its_check():
    assert all(c.check for c in tc.CASES if c.error is not None)


def test_stub_records_and_reads_taps():
    """The stub itself: a call is recorded with pointers as integers and the taps read through
    their pointer; the two size queries answer without counting as calls."""
    stub = tc.StubLib()
    h = np.array([7, -8, 9], np.int32)
    rc = stub.fir1d_fixed_rows_dev(ctypes.c_void_p(4096), 0, 2, 5, 1, h.ctypes.data_as(ctypes.c_void_p), 3, 12, 32, 1,
                                   ctypes.c_void_p(8192), ctypes.c_void_p(0))
    assert rc == 0 and stub.calls == [("fir1d_fixed_rows_dev", [4096, 0, 2, 5, 1, (7, -8, 9), 3, 12, 32, 1, 8192, 0])]
    assert stub.fir_restore_work_bytes() == tc.RESTORE_WORK and stub.fir_metrics_work_bytes(10) == tc.metrics_work(10)
    assert len(stub.calls) == 1 and len(stub.queries) == 2


def test_maker_alias_and_standin():
    """The stand-ins report what the tensors under them report, and Maker.alias places a tensor at
    the stated byte distance inside the other's allocation."""
    mk = tc.Maker(standin=True)
    x = mk.dev((3, 40), torch.uint8)
    assert x.is_cuda and x.device == torch.device("cuda:0") and x.is_contiguous() and x.dim() == 2
    assert tuple(x.shape) == (3, 40) and x.numel() == 120 and x.element_size() == 1 and x.dtype == torch.uint8
    y = mk.alias(x, 116, (3, 40), torch.int32)
    assert y.data_ptr() == x.data_ptr() + 116 and y.numel() * y.element_size() == 480
    assert not mk.strided((3, 40), torch.int16).is_contiguous()
    assert not mk.host((2,), torch.uint8).is_cuda and mk.other((2,), torch.uint8).device == torch.device("cuda:1")


def test_wrapped_bank_tap_changes_the_answer():
    """Why the bank taps go through _taps_i32: a plain int32 cast turns a tap of 2**31 into -2**31,
    and the oracle's outputs with the wrapped tap differ from those with the tap as given (exact
    in 64 bits: 9 taps, |x| <= 100, far below 2^63).  So "refused" and "silently wrapped" are
    different answers, and the device entries must give the first."""
    from oracle import fir_oracle as fo

    rng = np.random.default_rng(31)
    x = rng.integers(-100, 101, (5, 264)).astype(np.int16)
    h = rng.integers(-2000, 2001, 9).astype(np.int64)
    h[4] = 2**31
    wrapped = h.astype(np.int32).astype(np.int64)
    assert wrapped[4] == -2**31
    exact = fo.wrap_round(fo._mac_rows(x.astype(np.int64), h), 20, 64)
    assert not np.array_equal(exact, fo.wrap_round(fo._mac_rows(x.astype(np.int64), wrapped), 20, 64))
    with pytest.raises(fir_hip.FirHipError, match="must fit in int32"):
        torch_ops._bank_i32(np.stack([h, h]))
