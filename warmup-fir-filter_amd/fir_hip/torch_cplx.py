"""Device-tensor entry point of the complex-tap FIR (``fir_cplx_rows_dev`` of ``include/fir_hip.h``).

A module of its own beside :mod:`fir_hip.torch_ops`, whose helpers and conventions it shares, as
:mod:`fir_hip.torch_resample` does: the call is enqueued on the tensor's current stream (or
``stream``) and returns without synchronising.
"""
from __future__ import annotations

import ctypes

import torch

from . import OUT_I32, FirHipError, _check, _taps_cplx_i32, lib
from .torch_ops import _check_dev, _check_out, _no_overlap, _out_dtype, _rows_of, _stream_ptr

__all__ = ["CplxTaps", "fir1d_fixed_rows_cplx_dev"]


class CplxTaps:
    """Quantized complex taps kept as a (taps, 2) int32 array of (hr, hi) (no per-call conversion)."""

    def __init__(self, hq):
        self.h = _taps_cplx_i32(hq)
        self.ptr = self.h.ctypes.data_as(ctypes.c_void_p)
        self.n = int(self.h.shape[0])


def fir1d_fixed_rows_cplx_dev(x: torch.Tensor, hq, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32,
                              out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Row-wise 1-D fixed FIR of a complex int16 device tensor (last axis = one row of 2 * width
    interleaved (re, im) values) with the complex taps ``hq``, a (taps, 2) integer array of (hr, hi)
    or a CplxTaps (fir_cplx_rows_dev); returns a tensor of x's shape, int32 or uint8 per component.
    No conjugation and no gain; with every hi = 0 it equals fir1d_fixed_rows_dev(..., channels=2)."""
    _check_dev(x, "x")
    if x.dtype != torch.int16:
        raise FirHipError(f"x dtype must be int16 (interleaved re, im), got {x.dtype}")
    t = hq if isinstance(hq, CplxTaps) else CplxTaps(hq)
    rows, rowlen = _rows_of(x, 2)  # a 0-d x counts as a row of one value: refused as an odd row
    if out is None:
        out = torch.empty(x.shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, x.shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir_cplx_rows_dev(ctypes.c_void_p(x.data_ptr()), rows, rowlen // 2, t.ptr, t.n, int(frac_bits),
                                   int(acc_bits), int(out_stage), ctypes.c_void_p(out.data_ptr()),
                                   _stream_ptr(x, stream)), "fir_cplx_rows_dev")
    return out


def _cplx_rate_dev(ext, entry: str, x: torch.Tensor, hq, rates, frac_bits, acc_bits, out_stage, out, stream) -> torch.Tensor:
    """The device-tensor entry of a rate-changing complex-tap FIR: ``ext`` is its ctypes module
    (:mod:`fir_hip.cdecim`, :mod:`fir_hip.cinterp` or :mod:`fir_hip.cresample`), ``entry`` its
    fir_cplx_*_rows_dev and ``rates`` that entry's rate arguments, in its order and ext.out_width's."""
    _check_dev(x, "x")
    if x.dtype != torch.int16:
        raise FirHipError(f"x dtype must be int16 (interleaved re, im), got {x.dtype}")
    t = hq if isinstance(hq, CplxTaps) else CplxTaps(hq)
    rows, rowlen = _rows_of(x, 2)  # a 0-d x counts as a row of one value: refused as an odd row
    shape = tuple(x.shape[:-1]) + (2 * ext.out_width(rowlen // 2, *rates),)
    if out is None:
        out = torch.empty(shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    ext._check(getattr(ext.lib(), entry)(ctypes.c_void_p(x.data_ptr()), rows, rowlen // 2, t.ptr, t.n,
                                         *(int(v) for v in rates), int(frac_bits), int(acc_bits), int(out_stage),
                                         ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)), entry)
    return out
