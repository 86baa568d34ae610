"""ctypes binding of ``libfir_crstream.so`` — the streaming (block-continuous) rational U/D resampling
complex-tap FIR for complex int16, with carried history.

The C ABI is declared in ``include/fir_crstream.h``.  The library is an extension beside
``libfir_hip.so``: this module is the only place that loads it, it is loaded on first use (importing
:mod:`fir_hip` does not load it), and neither library needs the other.  Host-array entry:
:func:`fir1d_fixed_rows_cplx_resample_block` (NumPy in, NumPy out, synchronous); the device-tensor
entries are in :mod:`fir_hip.torch_crstream`.  :func:`route` says, without a device, which FIR kernel a
call would take, :func:`last_launch` which one the calling thread's last call did take.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import OUT_I32, OUT_U8_SAT, FirHipError, _ptr, _taps_cplx_i32
from ._ext import Ext, host_rows

__all__ = ["lib", "lib_path", "build_id", "out_width", "next_phase", "hist_frames", "route", "last_launch",
           "fir1d_fixed_rows_cplx_resample_block", "Route", "ROUTE_NONE", "ROUTE_FAST", "ROUTE_GENERIC32",
           "ROUTE_GENERIC64", "ROUTE_GENERIC128", "EXPORTS"]

ROUTE_NONE, ROUTE_FAST, ROUTE_GENERIC32, ROUTE_GENERIC64, ROUTE_GENERIC128 = range(5)  # FIR_CRSTREAM_*

_i32, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_uptr = ctypes.c_size_t  # uintptr_t
_pi32 = ctypes.POINTER(ctypes.c_int)

# symbol -> (restype, argtypes); mirrors include/fir_crstream.h one to one
EXPORTS = {
    "fir_crstream_build_id": (ctypes.c_char_p, []),
    "fir_crstream_last_error": (ctypes.c_char_p, []),
    "fir_cplx_rstream_out_width": (_i64, [_i64, _i32, _i32, _i32]),
    "fir_cplx_rstream_next_phase": (_i32, [_i64, _i32, _i32, _i32]),
    "fir_cplx_rstream_hist_frames": (_i32, [_i32, _i32]),
    "fir_cplx_rstream_block": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp,
                                      _i32]),
    "fir_cplx_rstream_block_dev": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp,
                                          _vp]),
    "fir_cplx_rstream_route": (_i32, [_uptr, _uptr, _uptr, _uptr, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                      _i32, _pi32]),
    "fir_cplx_rstream_last_launch": (_i32, [_pi32, _pi32]),
}

# the loader: libfir_crstream.so is loaded by the first lib() call, not on import
_ext = Ext("crstream", EXPORTS)
lib, lib_path, build_id, _check = _ext.lib, _ext.lib_path, _ext.build_id, _ext.check


class Route(NamedTuple):
    """A dispatch decision: ``route`` is one of ROUTE_*, ``tap_bucket`` the fast path's padded taps
    per phase (0 off the fast path)."""
    route: int
    tap_bucket: int


def _rate_args(width, up, decim, phase) -> tuple[int, int, int, int]:
    width, up, decim, phase = int(width), int(up), int(decim), int(phase)
    if up < 1:
        raise FirHipError("up must be >= 1")
    if decim < 1:
        raise FirHipError("decim must be >= 1")
    if not 0 <= phase < decim:
        raise FirHipError("phase must be in [0, decim)")
    if width < 0:
        raise FirHipError("width must be >= 0")
    return width, up, decim, phase


def out_width(width: int, up: int, decim: int, phase: int = 0) -> int:
    """Frames a block of ``width`` frames keeps when its first kept frame is frame ``phase`` of its
    ``width * up`` intermediate frames (fir_cplx_rstream_out_width); FirHipError for up < 1,
    decim < 1, a phase outside [0, decim) or a negative width.  Needs no library."""
    width, up, decim, phase = _rate_args(width, up, decim, phase)
    mid = width * up
    return (mid - phase + decim - 1) // decim if mid > phase else 0


def next_phase(width: int, up: int, decim: int, phase: int = 0) -> int:
    """The phase of the block that follows a block of ``width`` frames (fir_cplx_rstream_next_phase):
    ``phase + out_width * decim - width * up``, always in [0, decim).  Needs no library."""
    width, up, decim, phase = _rate_args(width, up, decim, phase)
    return phase + out_width(width, up, decim, phase) * decim - width * up


def hist_frames(taps: int, up: int) -> int:
    """H, the frames of history a row carries: ``(taps - 1) // up`` (fir_cplx_rstream_hist_frames).
    Needs no library."""
    taps, up = int(taps), int(up)
    if taps < 1:
        raise FirHipError("taps must be >= 1")
    if up < 1:
        raise FirHipError("up must be >= 1")
    return (taps - 1) // up


def route(x_addr: int, hist_in_addr: int, y_addr: int, hist_out_addr: int, rows: int, width: int, hq, up: int, decim: int,
          phase: int = 0, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32) -> Route:
    """The FIR kernel a call with these arguments would take (fir_cplx_rstream_route): the four
    addresses are those x, hist_in, y and hist_out would have (0: None), ``rows`` and ``width`` count
    frames.  Needs no device.  ROUTE_NONE when no FIR kernel runs; FirHipError for a call the library
    refuses."""
    return Route(*_ext.route4("fir_cplx_rstream_route", (x_addr, hist_in_addr, y_addr, hist_out_addr), rows, width, hq,
                              (up, decim, phase), frac_bits, acc_bits, out_stage))


def last_launch() -> Route:
    """The FIR kernel the calling thread's last fir_cplx_rstream_block[_dev] call that passed its
    checks launched (ROUTE_NONE: none; the history kernel is not reported)."""
    return Route(*_ext.last_launch("fir_cplx_rstream_last_launch"))


def fir1d_fixed_rows_cplx_resample_block(x: np.ndarray, hist, hq, up: int, decim: int, phase: int = 0,
                                         frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32,
                                         device: int = 0):
    """One block of each row's stream through the causal complex-tap resampler: zero-stuff by ``up``,
    filter, keep every ``decim``-th intermediate frame, the first at intermediate frame ``phase`` of
    the block (fir_cplx_rstream_block).  x's last axis holds 2 * width interleaved int16 (re, im)
    values, hq is a (taps, 2) integer array of (hr, hi); ``hist`` holds the H = (taps - 1) // up
    frames that precede x in every row (x's leading axes, a last axis of 2 * H int16 values, oldest
    first), None: zeros, the start of a stream.  Returns ``(y, hist_out, next_phase)``: y has x's
    leading axes and a last axis of 2 * out_width(width, up, decim, phase) values, int32 (OUT_I32) or
    uint8 (OUT_U8_SAT); hist_out and next_phase are the ``hist`` and ``phase`` of the next block.  The
    outputs of any split of a signal into blocks concatenate to the output of one block over the
    whole signal, bit for bit."""
    x, rows, rowlen = host_rows(x)
    h = _taps_cplx_i32(hq)
    width, up, decim, phase = _rate_args(rowlen // 2, up, decim, phase)
    H = hist_frames(h.shape[0], up)
    hshape = x.shape[:-1] + (2 * H,)
    if hist is not None:
        if not isinstance(hist, np.ndarray) or hist.dtype != np.int16:
            raise FirHipError(f"hist must be an int16 array of interleaved (re, im), got "
                              f"{getattr(hist, 'dtype', type(hist).__name__)}")
        if hist.shape != hshape:
            raise FirHipError(f"hist must have shape {hshape} (x's leading axes, 2 * ((taps - 1) // up) values), got "
                              f"{hist.shape}")
        hist = np.ascontiguousarray(hist)
    ow = out_width(width, up, decim, phase)
    if rowlen == 0:  # host_rows counts no rows for rows of no values; the history still moves
        rows = int(np.prod(x.shape[:-1], dtype=np.int64))
    y = np.empty(x.shape[:-1] + (2 * ow,), np.uint8 if out_stage == OUT_U8_SAT else np.int32)
    hist_out = np.empty(hshape, np.int16)
    _check(lib().fir_cplx_rstream_block(_ptr(x), None if hist is None else _ptr(hist), rows, width, _ptr(h), h.shape[0],
                                        up, decim, phase, int(frac_bits), int(acc_bits), int(out_stage), _ptr(y),
                                        _ptr(hist_out), int(device)), "fir_cplx_rstream_block")
    return y, hist_out, next_phase(width, up, decim, phase)
