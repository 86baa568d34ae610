"""Device-tensor entry point of the resampling FIR (``fir_resample_rows_dev`` of ``include/fir_hip.h``).

A module of its own beside :mod:`fir_hip.torch_ops`, whose helpers and conventions it shares, as
:mod:`fir_hip.torch_interp` does: the call is enqueued on the tensor's current stream (or
``stream``) and returns without synchronising.
"""
from __future__ import annotations

import ctypes

import torch

from . import OUT_I32, FirHipError, _check, lib, resample_out_width
from .torch_ops import _IN, _check_dev, _check_out, _no_overlap, _out_dtype, _rows_of, _stream_ptr, _taps

__all__ = ["fir1d_fixed_rows_resample_dev"]


def fir1d_fixed_rows_resample_dev(x: torch.Tensor, hq, up: int, decim: int, phase: int = 0, frac_bits: int = 12,
                                  acc_bits: int = 32, out_stage: int = OUT_I32, channels: int = 1,
                                  out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """fir1d_fixed_rows_interp_dev(x, hq, up, ...) viewed as (..., width * up, channels)
    ``[..., phase::decim, :]`` (fir_resample_rows_dev): x's leading axes with a last axis of
    resample_out_width(width, up, decim, phase) * channels values.  One pass in polyphase form: x
    is read once, the interpolated signal is never stored and no dropped frame is computed.  There
    is no gain: for unity passband gain scale the taps by ``up``."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    t = _taps(hq)
    rows, rowlen = _rows_of(x, channels)
    ow = resample_out_width(rowlen // channels, up, decim, phase)
    shape = tuple(x.shape[:-1]) + (ow * channels,)
    if out is None:
        out = torch.empty(shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir_resample_rows_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], rows, rowlen // channels, channels,
                                       t.ptr, t.n, int(up), int(decim), int(phase), int(frac_bits), int(acc_bits),
                                       int(out_stage), ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir_resample_rows_dev")
    return out
