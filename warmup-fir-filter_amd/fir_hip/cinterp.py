"""ctypes binding of ``libfir_cinterp.so`` — the interpolating complex-tap FIR for complex int16.

The C ABI is declared in ``include/fir_cinterp.h``.  The library is an extension beside
``libfir_hip.so`` and ``libfir_cdecim.so``: this module is the only place that loads it, it is loaded
on first use (importing :mod:`fir_hip` does not load it), and no library needs another.  Host-array
entry: :func:`fir1d_fixed_rows_cplx_interp` (NumPy in, NumPy out, synchronous); the device-tensor
entry is in :mod:`fir_hip.torch_cinterp`.  :func:`route` says, without a device, which kernel a call
would take, :func:`last_launch` which one the calling thread's last call did take.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import OUT_I32, OUT_U8_SAT, FirHipError, _out_buf, _ptr, _taps_cplx_i32
from ._ext import Ext, host_rows

__all__ = ["lib", "lib_path", "build_id", "out_width", "route", "last_launch", "fir1d_fixed_rows_cplx_interp",
           "Route", "ROUTE_NONE", "ROUTE_FAST", "ROUTE_GENERIC32", "ROUTE_GENERIC64", "ROUTE_GENERIC128", "EXPORTS"]

ROUTE_NONE, ROUTE_FAST, ROUTE_GENERIC32, ROUTE_GENERIC64, ROUTE_GENERIC128 = range(5)  # FIR_CINTERP_*

_i32, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_uptr = ctypes.c_size_t  # uintptr_t
_pi32 = ctypes.POINTER(ctypes.c_int)

# symbol -> (restype, argtypes); mirrors include/fir_cinterp.h one to one
EXPORTS = {
    "fir_cinterp_build_id": (ctypes.c_char_p, []),
    "fir_cinterp_last_error": (ctypes.c_char_p, []),
    "fir_cplx_interp_out_width": (_i64, [_i64, _i32]),
    "fir_cplx_interp_rows": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32]),
    "fir_cplx_interp_rows_dev": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "fir_cplx_interp_route": (_i32, [_uptr, _uptr, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _pi32]),
    "fir_cplx_interp_last_launch": (_i32, [_pi32, _pi32]),
}

# the loader: libfir_cinterp.so is loaded by the first lib() call, not on import
_ext = Ext("cinterp", EXPORTS)
lib, lib_path, build_id, _check = _ext.lib, _ext.lib_path, _ext.build_id, _ext.check


class Route(NamedTuple):
    """A dispatch decision: ``route`` is one of ROUTE_*, ``window_bucket`` the fast path's padded
    window length per phase (0 off the fast path)."""
    route: int
    window_bucket: int


def out_width(width: int, up: int) -> int:
    """Frames a row of ``width`` frames has after zero-stuffing by ``up`` (fir_cplx_interp_out_width):
    width * up; FirHipError for up < 1, a negative width or a product past int64.  Needs no library."""
    width, up = int(width), int(up)
    if up < 1:
        raise FirHipError("up must be >= 1")
    if width < 0:
        raise FirHipError("width must be >= 0")
    if width * up >= 1 << 63:
        raise FirHipError("width * up does not fit in int64")
    return width * up


def route(x_addr: int, y_addr: int, rows: int, width: int, hq, up: int, frac_bits: int = 12, acc_bits: int = 32,
          out_stage: int = OUT_I32) -> Route:
    """The kernel a call with these arguments would take (fir_cplx_interp_route): ``x_addr`` and
    ``y_addr`` are the addresses x and y would have, ``rows`` and ``width`` count frames.  Needs no
    device.  ROUTE_NONE for an empty problem; FirHipError for a call the library refuses."""
    return Route(*_ext.route("fir_cplx_interp_route", x_addr, y_addr, rows, width, hq, (up,), frac_bits, acc_bits,
                             out_stage))


def last_launch() -> Route:
    """What the calling thread's last fir_cplx_interp_rows[_dev] call that passed its checks
    launched (ROUTE_NONE: nothing)."""
    return Route(*_ext.last_launch("fir_cplx_interp_last_launch"))


def fir1d_fixed_rows_cplx_interp(x: np.ndarray, hq, up: int, frac_bits: int = 12, acc_bits: int = 32,
                                 out_stage: int = OUT_I32, device: int = 0,
                                 out: np.ndarray | None = None) -> np.ndarray:
    """The interpolating complex-tap FIR: the value of ``fir1d_fixed_rows_cplx`` for x with ``up - 1``
    zero frames stuffed after every frame (viewed as (..., width, 2): ``xu[..., ::up, :] = x``),
    computed in polyphase form from x itself, so no stuffed signal is stored and no tap meets a
    stuffed zero.  x's last axis holds 2 * width interleaved int16 (re, im) values, hq is a (taps, 2)
    integer array of (hr, hi).  Returns x's leading axes with a last axis of 2 * width * up values,
    int32 (OUT_I32) or uint8 (OUT_U8_SAT).  There is no gain: for unity passband gain scale the taps
    by ``up`` before quantizing them."""
    x, rows, rowlen = host_rows(x)
    h = _taps_cplx_i32(hq)
    ow = out_width(rowlen // 2, up)
    y = _out_buf(out, x.shape[:-1] + (2 * ow,), np.uint8 if out_stage == OUT_U8_SAT else np.int32, x)
    _check(lib().fir_cplx_interp_rows(_ptr(x), rows, rowlen // 2, _ptr(h), h.shape[0], int(up), int(frac_bits),
                                      int(acc_bits), int(out_stage), _ptr(y), int(device)),
           "fir_cplx_interp_rows")
    return y
