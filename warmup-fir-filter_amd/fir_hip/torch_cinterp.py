"""Device-tensor entry point of the interpolating complex-tap FIR (``fir_cplx_interp_rows_dev`` of
``include/fir_cinterp.h``, in the extension library that :mod:`fir_hip.cinterp` loads).

It shares the helpers and conventions of :mod:`fir_hip.torch_ops`, as :mod:`fir_hip.torch_cdecim`
does: the call is enqueued on the tensor's current stream (or ``stream``) and returns without
synchronising.
"""
from __future__ import annotations

import torch

from . import OUT_I32, cinterp
from .torch_cplx import CplxTaps, _cplx_rate_dev

__all__ = ["CplxTaps", "fir1d_fixed_rows_cplx_interp_dev"]


def fir1d_fixed_rows_cplx_interp_dev(x: torch.Tensor, hq, up: int, frac_bits: int = 12, acc_bits: int = 32,
                                     out_stage: int = OUT_I32, out: torch.Tensor | None = None,
                                     stream=None) -> torch.Tensor:
    """fir1d_fixed_rows_cplx_dev of x zero-stuffed by ``up``, computed in polyphase form from x itself
    (fir_cplx_interp_rows_dev).  x: a complex int16 device tensor (last axis = one row of 2 * width
    interleaved (re, im) values); hq: a (taps, 2) integer array of (hr, hi) or a CplxTaps.  Returns
    x's leading axes with a last axis of 2 * width * up values, int32 or uint8 per component."""
    return _cplx_rate_dev(cinterp, "fir_cplx_interp_rows_dev", x, hq, (up,), frac_bits, acc_bits,
                          out_stage, out, stream)
