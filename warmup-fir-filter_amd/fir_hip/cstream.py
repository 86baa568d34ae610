"""ctypes binding of ``libfir_cstream.so`` — the streaming (block-continuous) decimating complex-tap
FIR for complex int16, with carried history.

The C ABI is declared in ``include/fir_cstream.h``.  The library is an extension beside
``libfir_hip.so``: this module is the only place that loads it, it is loaded on first use (importing
:mod:`fir_hip` does not load it), and neither library needs the other.  Host-array entry:
:func:`fir1d_fixed_rows_cplx_decim_block` (NumPy in, NumPy out, synchronous); the device-tensor
entries are in :mod:`fir_hip.torch_cstream`.  :func:`route` says, without a device, which FIR kernel a
call would take, :func:`last_launch` which one the calling thread's last call did take.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import OUT_I32, OUT_U8_SAT, FirHipError, _ptr, _taps_cplx_i32
from ._ext import Ext, host_rows

__all__ = ["lib", "lib_path", "build_id", "out_width", "next_phase", "route", "last_launch",
           "fir1d_fixed_rows_cplx_decim_block", "Route", "ROUTE_NONE", "ROUTE_FAST", "ROUTE_GENERIC32",
           "ROUTE_GENERIC64", "ROUTE_GENERIC128", "EXPORTS"]

ROUTE_NONE, ROUTE_FAST, ROUTE_GENERIC32, ROUTE_GENERIC64, ROUTE_GENERIC128 = range(5)  # FIR_CSTREAM_*

_i32, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_uptr = ctypes.c_size_t  # uintptr_t
_pi32 = ctypes.POINTER(ctypes.c_int)

# symbol -> (restype, argtypes); mirrors include/fir_cstream.h one to one
EXPORTS = {
    "fir_cstream_build_id": (ctypes.c_char_p, []),
    "fir_cstream_last_error": (ctypes.c_char_p, []),
    "fir_cplx_stream_out_width": (_i64, [_i64, _i32, _i32]),
    "fir_cplx_stream_next_phase": (_i32, [_i64, _i32, _i32]),
    "fir_cplx_stream_block": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32]),
    "fir_cplx_stream_block_dev": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "fir_cplx_stream_route": (_i32, [_uptr, _uptr, _uptr, _uptr, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                     _pi32]),
    "fir_cplx_stream_last_launch": (_i32, [_pi32, _pi32]),
}

# the loader: libfir_cstream.so is loaded by the first lib() call, not on import
_ext = Ext("cstream", EXPORTS)
lib, lib_path, build_id, _check = _ext.lib, _ext.lib_path, _ext.build_id, _ext.check


class Route(NamedTuple):
    """A dispatch decision: ``route`` is one of ROUTE_*, ``tap_bucket`` the fast path's padded tap
    count (0 off the fast path)."""
    route: int
    tap_bucket: int


def _rate_args(width, decim, phase) -> tuple[int, int, int]:
    width, decim, phase = int(width), int(decim), int(phase)
    if decim < 1:
        raise FirHipError("decim must be >= 1")
    if not 0 <= phase < decim:
        raise FirHipError("phase must be in [0, decim)")
    if width < 0:
        raise FirHipError("width must be >= 0")
    return width, decim, phase


def out_width(width: int, decim: int, phase: int = 0) -> int:
    """Frames a block of ``width`` frames keeps when its first kept frame is frame ``phase``
    (fir_cplx_stream_out_width); FirHipError for decim < 1, a phase outside [0, decim) or a negative
    width.  Needs no library."""
    width, decim, phase = _rate_args(width, decim, phase)
    return (width - phase + decim - 1) // decim if width > phase else 0


def next_phase(width: int, decim: int, phase: int = 0) -> int:
    """The phase of the block that follows a block of ``width`` frames (fir_cplx_stream_next_phase):
    ``phase + out_width * decim - width``, always in [0, decim).  Needs no library."""
    width, decim, phase = _rate_args(width, decim, phase)
    return phase + out_width(width, decim, phase) * decim - width


def route(x_addr: int, hist_in_addr: int, y_addr: int, hist_out_addr: int, rows: int, width: int, hq, decim: int,
          phase: int = 0, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32) -> Route:
    """The FIR kernel a call with these arguments would take (fir_cplx_stream_route): the four
    addresses are those x, hist_in, y and hist_out would have (0: None), ``rows`` and ``width`` count
    frames.  Needs no device.  ROUTE_NONE when no FIR kernel runs; FirHipError for a call the library
    refuses."""
    return Route(*_ext.route4("fir_cplx_stream_route", (x_addr, hist_in_addr, y_addr, hist_out_addr), rows, width, hq,
                              (decim, phase), frac_bits, acc_bits, out_stage))


def last_launch() -> Route:
    """The FIR kernel the calling thread's last fir_cplx_stream_block[_dev] call that passed its
    checks launched (ROUTE_NONE: none; the history kernel is not reported)."""
    return Route(*_ext.last_launch("fir_cplx_stream_last_launch"))


def fir1d_fixed_rows_cplx_decim_block(x: np.ndarray, hist, hq, decim: int, phase: int = 0, frac_bits: int = 12,
                                      acc_bits: int = 32, out_stage: int = OUT_I32, device: int = 0):
    """One block of each row's stream through the causal complex-tap FIR that keeps every ``decim``-th
    output frame, the first at frame ``phase`` of the block (fir_cplx_stream_block).  x's last axis
    holds 2 * width interleaved int16 (re, im) values, hq is a (taps, 2) integer array of (hr, hi);
    ``hist`` holds the taps - 1 frames that precede x in every row (x's leading axes, a last axis of
    2 * (taps - 1) int16 values, oldest first), None: zeros, the start of a stream.  Returns
    ``(y, hist_out, next_phase)``: y has x's leading axes and a last axis of
    2 * out_width(width, decim, phase) values, int32 (OUT_I32) or uint8 (OUT_U8_SAT); hist_out and
    next_phase are the ``hist`` and ``phase`` of the next block.  The outputs of any split of a
    signal into blocks concatenate to the output of one block over the whole signal, bit for bit."""
    x, rows, rowlen = host_rows(x)
    h = _taps_cplx_i32(hq)
    H = h.shape[0] - 1
    hshape = x.shape[:-1] + (2 * H,)
    if hist is not None:
        if not isinstance(hist, np.ndarray) or hist.dtype != np.int16:
            raise FirHipError(f"hist must be an int16 array of interleaved (re, im), got "
                              f"{getattr(hist, 'dtype', type(hist).__name__)}")
        if hist.shape != hshape:
            raise FirHipError(f"hist must have shape {hshape} (x's leading axes, 2 * (taps - 1) values), got {hist.shape}")
        hist = np.ascontiguousarray(hist)
    width = rowlen // 2
    ow = out_width(width, decim, phase)
    if rowlen == 0:  # host_rows counts no rows for rows of no values; the history still moves
        rows = int(np.prod(x.shape[:-1], dtype=np.int64))
    y = np.empty(x.shape[:-1] + (2 * ow,), np.uint8 if out_stage == OUT_U8_SAT else np.int32)
    hist_out = np.empty(hshape, np.int16)
    _check(lib().fir_cplx_stream_block(_ptr(x), None if hist is None else _ptr(hist), rows, width, _ptr(h), h.shape[0],
                                       int(decim), int(phase), int(frac_bits), int(acc_bits), int(out_stage), _ptr(y),
                                       _ptr(hist_out), int(device)), "fir_cplx_stream_block")
    return y, hist_out, next_phase(width, decim, phase)
