"""ctypes binding of ``libfir_cresample.so`` — the rational U/D resampling complex-tap FIR for complex
int16.

The C ABI is declared in ``include/fir_cresample.h``.  The library is an extension beside
``libfir_hip.so``, ``libfir_cdecim.so`` and ``libfir_cinterp.so``: this module is the only place that
loads it, it is loaded on first use (importing :mod:`fir_hip` does not load it), and no library needs
another.  Host-array entry: :func:`fir1d_fixed_rows_cplx_resample` (NumPy in, NumPy out,
synchronous); the device-tensor entry is in :mod:`fir_hip.torch_cresample`.  :func:`route` says,
without a device, which kernel a call would take, :func:`last_launch` which one the calling thread's
last call did take.  Calls with ``up = 1`` or ``decim = 1`` are legal and take the generic kernels:
the tuned entries for them are :mod:`fir_hip.cdecim` and :mod:`fir_hip.cinterp`.
"""
from __future__ import annotations

import ctypes
import threading
from pathlib import Path
from typing import NamedTuple

import numpy as np

from . import (OUT_I32, OUT_U8_SAT, FirHipError, _out_buf, _ptr, _share_torch_hip_runtime, _taps_cplx_i32)

__all__ = ["lib", "lib_path", "build_id", "out_width", "route", "last_launch", "fir1d_fixed_rows_cplx_resample",
           "Route", "ROUTE_NONE", "ROUTE_FAST", "ROUTE_GENERIC32", "ROUTE_GENERIC64", "ROUTE_GENERIC128", "EXPORTS"]

ROUTE_NONE, ROUTE_FAST, ROUTE_GENERIC32, ROUTE_GENERIC64, ROUTE_GENERIC128 = range(5)  # FIR_CRESAMPLE_*

_i32, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_uptr = ctypes.c_size_t  # uintptr_t
_pi32 = ctypes.POINTER(ctypes.c_int)

# symbol -> (restype, argtypes); mirrors include/fir_cresample.h one to one
EXPORTS = {
    "fir_cresample_build_id": (ctypes.c_char_p, []),
    "fir_cresample_last_error": (ctypes.c_char_p, []),
    "fir_cplx_resample_out_width": (_i64, [_i64, _i32, _i32, _i32]),
    "fir_cplx_resample_rows": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32]),
    "fir_cplx_resample_rows_dev": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "fir_cplx_resample_route": (_i32, [_uptr, _uptr, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _pi32]),
    "fir_cplx_resample_last_launch": (_i32, [_pi32, _pi32]),
}

_HERE = Path(__file__).resolve().parent
_lib = None
_lock = threading.Lock()


class Route(NamedTuple):
    """A dispatch decision: ``route`` is one of ROUTE_*, ``tap_bucket`` the fast path's padded
    sub-filter length per phase (0 off the fast path)."""
    route: int
    tap_bucket: int


def lib_path() -> Path:
    return _HERE / "libfir_cresample.so"


def lib() -> ctypes.CDLL:
    """Load libfir_cresample.so once; raise FirHipError if it is missing or built from other sources."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not path.exists():
            raise FirHipError(
                f"{path} is not built: run `make -C warmup-fir-filter_amd/csrc_cresample` or "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
        _share_torch_hip_runtime()
        try:
            handle = ctypes.CDLL(str(path))
        except OSError as exc:
            raise FirHipError(f"cannot load {path}: {exc}") from exc
        for name, (res, args) in EXPORTS.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as exc:
                raise FirHipError(f"{path} does not export {name}") from exc
            fn.restype = res
            fn.argtypes = args
        from ._srcid_cresample import source_id

        built, want = handle.fir_cresample_build_id().decode(), source_id()
        if want is not None and built != want:
            raise FirHipError(f"{path} was built from other sources (build id {built}, the sources beside it hash "
                              f"to {want}): rebuild with `make -C warmup-fir-filter_amd/csrc_cresample`")
        _lib = handle
    return _lib


def build_id() -> str:
    return lib().fir_cresample_build_id().decode()


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().fir_cresample_last_error().decode(errors="replace")
        raise FirHipError(f"{what} failed (status {rc}): {msg}")


def out_width(width: int, up: int, decim: int, phase: int = 0) -> int:
    """Frames a row of ``width`` frames has after resampling by ``up / decim`` at ``phase``
    (fir_cplx_resample_out_width): ceil((width * up - phase) / decim), 0 when width * up <= phase;
    FirHipError for up < 1, decim < 1, a phase outside [0, decim), a negative width or a width * up
    past int64.  Needs no library."""
    width, up, decim, phase = int(width), int(up), int(decim), int(phase)
    if up < 1:
        raise FirHipError("up must be >= 1")
    if decim < 1:
        raise FirHipError("decim must be >= 1")
    if not 0 <= phase < decim:
        raise FirHipError("phase must be in [0, decim)")
    if width < 0:
        raise FirHipError("width must be >= 0")
    mid = width * up
    if mid >= 1 << 63:
        raise FirHipError("width * up does not fit in int64")
    return -(-(mid - phase) // decim) if mid > phase else 0


def route(x_addr: int, y_addr: int, rows: int, width: int, hq, up: int, decim: int, phase: int = 0,
          frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_I32) -> Route:
    """The kernel a call with these arguments would take (fir_cplx_resample_route): ``x_addr`` and
    ``y_addr`` are the addresses x and y would have, ``rows`` and ``width`` count frames.  Needs no
    device.  ROUTE_NONE for an empty problem; FirHipError for a call the library refuses."""
    h = _taps_cplx_i32(hq)
    bucket = ctypes.c_int(0)
    r = lib().fir_cplx_resample_route(int(x_addr), int(y_addr), int(rows), int(width), _ptr(h), h.shape[0], int(up),
                                      int(decim), int(phase), int(frac_bits), int(acc_bits), int(out_stage),
                                      ctypes.byref(bucket))
    if r < 0:
        raise FirHipError("fir_cplx_resample_route refused the call: " +
                          lib().fir_cresample_last_error().decode(errors="replace"))
    return Route(r, bucket.value)


def last_launch() -> Route:
    """What the calling thread's last fir_cplx_resample_rows[_dev] call that passed its checks
    launched (ROUTE_NONE: nothing)."""
    r, bucket = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().fir_cplx_resample_last_launch(ctypes.byref(r), ctypes.byref(bucket)), "fir_cplx_resample_last_launch")
    return Route(r.value, bucket.value)


def fir1d_fixed_rows_cplx_resample(x: np.ndarray, hq, up: int, decim: int, phase: int = 0, frac_bits: int = 12,
                                   acc_bits: int = 32, out_stage: int = OUT_I32, device: int = 0,
                                   out: np.ndarray | None = None) -> np.ndarray:
    """The rational resampling complex-tap FIR: frames ``phase, phase + decim, ...`` of what
    ``fir1d_fixed_rows_cplx_interp(x, hq, up, ...)`` gives, computed in polyphase form from x itself,
    so no stuffed signal or intermediate is stored, no tap meets a stuffed zero and no dropped frame
    is computed.  x's last axis holds 2 * width interleaved int16 (re, im) values, hq is a (taps, 2)
    integer array of (hr, hi).  Returns x's leading axes with a last axis of
    2 * out_width(width, up, decim, phase) values, int32 (OUT_I32) or uint8 (OUT_U8_SAT).  There is no
    gain: for unity passband gain scale the taps by ``up`` before quantizing them."""
    if not isinstance(x, np.ndarray) or x.dtype != np.int16:
        raise FirHipError(f"x must be an int16 array of interleaved (re, im), got {getattr(x, 'dtype', type(x).__name__)}")
    if x.ndim == 0:
        raise FirHipError("x must have at least one axis of interleaved (re, im) values")
    if x.shape[-1] % 2:
        raise FirHipError(f"x's last axis must hold an even number of values (re, im pairs), got {x.shape[-1]}")
    x = np.ascontiguousarray(x)
    h = _taps_cplx_i32(hq)
    rowlen = x.shape[-1]
    rows = x.size // rowlen if rowlen else 0
    ow = out_width(rowlen // 2, up, decim, phase)
    y = _out_buf(out, x.shape[:-1] + (2 * ow,), np.uint8 if out_stage == OUT_U8_SAT else np.int32, x)
    _check(lib().fir_cplx_resample_rows(_ptr(x), rows, rowlen // 2, _ptr(h), h.shape[0], int(up), int(decim),
                                        int(phase), int(frac_bits), int(acc_bits), int(out_stage), _ptr(y), int(device)),
           "fir_cplx_resample_rows")
    return y
