"""Device-tensor entry points of the streaming rational U/D resampling complex-tap FIR
(``fir_cplx_rstream_block_dev`` of ``include/fir_crstream.h``, in the extension library that
:mod:`fir_hip.crstream` loads).

They share the helpers and conventions of :mod:`fir_hip.torch_ops`, as :mod:`fir_hip.torch_cstream`
does: a call is enqueued on the tensor's current stream (or ``stream``) and returns without
synchronising.  :func:`fir1d_fixed_rows_cplx_resample_block_dev` is stateless (the caller owns both
history buffers and the phase); :class:`CplxResampleStream` owns them.
"""
from __future__ import annotations

import ctypes

import torch

from . import OUT_I32, FirHipError, crstream
from .torch_cplx import CplxTaps
from .torch_ops import _check_dev, _check_in, _check_out, _no_overlap, _out_dtype, _rows_of, _stream_ptr

__all__ = ["CplxTaps", "CplxResampleStream", "fir1d_fixed_rows_cplx_resample_block_dev"]


def _opt_ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def fir1d_fixed_rows_cplx_resample_block_dev(x: torch.Tensor, hist_in, hist_out, hq, up: int, decim: int, phase: int = 0,
                                             frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32,
                                             out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """One block of each row's stream through the causal complex-tap resampler: zero-stuff by ``up``,
    filter, keep every ``decim``-th intermediate frame, the first at intermediate frame ``phase`` of
    the block (fir_cplx_rstream_block_dev).  x: a complex int16 device tensor (last axis = one row of
    2 * width interleaved (re, im) values); hq: a (taps, 2) integer array of (hr, hi) or a CplxTaps.
    ``hist_in``: the H = (taps - 1) // up frames that precede x in every row (int16, x's leading
    axes, a last axis of 2 * H values, oldest first), None: zeros.  ``hist_out``: a tensor of the same
    shape that receives the history of the next block (it must not overlap hist_in, x or out), None:
    nothing is written.  Returns x's leading axes with a last axis of
    2 * out_width(width, up, decim, phase) values, int32 or uint8 per component; the next block's
    phase is ``crstream.next_phase(width, up, decim, phase)``."""
    _check_dev(x, "x")
    if x.dtype != torch.int16:
        raise FirHipError(f"x dtype must be int16 (interleaved re, im), got {x.dtype}")
    t = hq if isinstance(hq, CplxTaps) else CplxTaps(hq)
    rows, rowlen = _rows_of(x, 2)  # a 0-d x counts as a row of one value: refused as an odd row
    lead = tuple(x.shape[:-1])
    if rowlen == 0:  # rows of no frames: the history still moves
        rows = 1
        for n in lead:
            rows *= n
    shape = lead + (2 * crstream.out_width(rowlen // 2, up, decim, phase),)  # refuses a bad up, decim or phase
    hshape = lead + (2 * crstream.hist_frames(t.n, up),)
    if hist_in is not None:
        _check_in(hist_in, x, "hist_in")
        if tuple(hist_in.shape) != hshape or hist_in.dtype != torch.int16:
            raise FirHipError(f"hist_in must be {torch.int16} of shape {hshape}, got {hist_in.dtype} of shape "
                              f"{tuple(hist_in.shape)}")
    if hist_out is not None:
        _check_out(hist_out, hshape, torch.int16, x, "hist_out")
    if out is None:
        out = torch.empty(shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)] + ([("hist_in", hist_in)] if hist_in is not None else []),
                [("out", out)] + ([("hist_out", hist_out)] if hist_out is not None else []))
    crstream._check(crstream.lib().fir_cplx_rstream_block_dev(
        ctypes.c_void_p(x.data_ptr()), _opt_ptr(hist_in), rows, rowlen // 2, t.ptr, t.n, int(up), int(decim), int(phase),
        int(frac_bits), int(acc_bits), int(out_stage), ctypes.c_void_p(out.data_ptr()), _opt_ptr(hist_out),
        _stream_ptr(x, stream)), "fir_cplx_rstream_block_dev")
    return out


class CplxResampleStream:
    """A stream (or ``lead_shape`` independent streams) through the causal U/D resampling complex-tap
    FIR: the object owns the two history tensors it ping-pongs between and the phase, so that the
    outputs of successive :meth:`push` calls concatenate, bit for bit, to the output of one call over
    the whole signal.

    Pushes of one object must be stream-ordered by the caller: every push reads the history the
    push before it wrote, so they go to one stream, or the caller orders the streams with events.
    Nothing here synchronises."""

    def __init__(self, hq, up: int, decim: int, lead_shape=(), *, phase: int = 0, frac_bits: int = 12,
                 acc_bits: int = 32, out_stage: int = OUT_I32, device):
        self.taps = hq if isinstance(hq, CplxTaps) else CplxTaps(hq)
        self.up, self.decim = int(up), int(decim)
        self.frac_bits, self.acc_bits, self.out_stage = int(frac_bits), int(acc_bits), int(out_stage)
        self.lead_shape = tuple(int(n) for n in lead_shape)
        self.device = torch.device(device)
        _out_dtype(self.out_stage)
        crstream.out_width(0, self.up, self.decim, phase)  # refuses a bad up, decim or phase
        self.hist_frames = crstream.hist_frames(self.taps.n, self.up)
        hshape = self.lead_shape + (2 * self.hist_frames,)
        self._hist = [torch.zeros(hshape, dtype=torch.int16, device=self.device) for _ in range(2)]
        self._cur = 0
        self._phase = int(phase)
        self._frames_in = self._frames_out = 0

    @property
    def phase(self) -> int:
        """The index, in the next block's intermediate frames, of its first kept frame."""
        return self._phase

    @property
    def history(self) -> torch.Tensor:
        """A copy of the (taps - 1) // up frames that precede the next block (enqueued, not synchronised)."""
        return self._hist[self._cur].clone()

    @property
    def frames_in(self) -> int:
        """Frames pushed per row since the last reset."""
        return self._frames_in

    @property
    def frames_out(self) -> int:
        """Frames returned per row since the last reset."""
        return self._frames_out

    def reset(self, history: torch.Tensor | None = None, phase: int = 0) -> None:
        """Start the stream again: a zero history (or a copy of ``history``) and ``phase``."""
        crstream.out_width(0, self.up, self.decim, phase)
        cur = self._hist[self._cur]
        if history is None:
            cur.zero_()
        else:
            if tuple(history.shape) != tuple(cur.shape) or history.dtype != torch.int16:
                raise FirHipError(f"history must be {torch.int16} of shape {tuple(cur.shape)}, got {history.dtype} of "
                                  f"shape {tuple(history.shape)}")
            cur.copy_(history)
        self._phase = int(phase)
        self._frames_in = self._frames_out = 0

    def push(self, x: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """Resample the next block (any width >= 0; x's leading axes must equal ``lead_shape``) and
        carry the history and the phase on."""
        if tuple(x.shape[:-1]) != self.lead_shape or x.dim() == 0:
            raise FirHipError(f"x's leading axes must be {self.lead_shape}, got "
                              f"{tuple(x.shape[:-1]) if x.dim() else 'a 0-d tensor'}")
        nxt = 1 - self._cur
        y = fir1d_fixed_rows_cplx_resample_block_dev(x, self._hist[self._cur], self._hist[nxt], self.taps, self.up,
                                                     self.decim, self._phase, self.frac_bits, self.acc_bits,
                                                     self.out_stage, out, stream)
        width = x.shape[-1] // 2
        self._phase = crstream.next_phase(width, self.up, self.decim, self._phase)
        self._frames_in += width
        self._frames_out += y.shape[-1] // 2
        if self.hist_frames > 0:
            self._cur = nxt
        return y
