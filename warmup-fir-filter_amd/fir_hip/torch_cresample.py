"""Device-tensor entry point of the rational resampling complex-tap FIR
(``fir_cplx_resample_rows_dev`` of ``include/fir_cresample.h``, in the extension library that
:mod:`fir_hip.cresample` loads).

It shares the helpers and conventions of :mod:`fir_hip.torch_ops`, as :mod:`fir_hip.torch_cinterp`
does: the call is enqueued on the tensor's current stream (or ``stream``) and returns without
synchronising.
"""
from __future__ import annotations

import ctypes

import torch

from . import OUT_I32, FirHipError
from .cresample import _check, lib, out_width
from .torch_cplx import CplxTaps
from .torch_ops import _check_dev, _check_out, _no_overlap, _out_dtype, _rows_of, _stream_ptr

__all__ = ["CplxTaps", "fir1d_fixed_rows_cplx_resample_dev"]


def fir1d_fixed_rows_cplx_resample_dev(x: torch.Tensor, hq, up: int, decim: int, phase: int = 0, frac_bits: int = 12,
                                       acc_bits: int = 32, out_stage: int = OUT_I32, out: torch.Tensor | None = None,
                                       stream=None) -> torch.Tensor:
    """Frames ``phase, phase + decim, ...`` of fir1d_fixed_rows_cplx_interp_dev(x, hq, up), computed in
    one polyphase pass from x itself (fir_cplx_resample_rows_dev).  x: a complex int16 device tensor
    (last axis = one row of 2 * width interleaved (re, im) values); hq: a (taps, 2) integer array of
    (hr, hi) or a CplxTaps.  Returns x's leading axes with a last axis of
    2 * out_width(width, up, decim, phase) values, int32 or uint8 per component."""
    _check_dev(x, "x")
    if x.dtype != torch.int16:
        raise FirHipError(f"x dtype must be int16 (interleaved re, im), got {x.dtype}")
    t = hq if isinstance(hq, CplxTaps) else CplxTaps(hq)
    rows, rowlen = _rows_of(x, 2)  # a 0-d x counts as a row of one value: refused as an odd row
    shape = tuple(x.shape[:-1]) + (2 * out_width(rowlen // 2, up, decim, phase),)
    if out is None:
        out = torch.empty(shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir_cplx_resample_rows_dev(ctypes.c_void_p(x.data_ptr()), rows, rowlen // 2, t.ptr, t.n, int(up),
                                            int(decim), int(phase), int(frac_bits), int(acc_bits), int(out_stage),
                                            ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir_cplx_resample_rows_dev")
    return out
