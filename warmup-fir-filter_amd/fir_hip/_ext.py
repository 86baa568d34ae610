"""The loader the extension libraries' ctypes modules share (:mod:`fir_hip.cdecim`,
:mod:`fir_hip.cinterp`, :mod:`fir_hip.cresample`, :mod:`fir_hip.cstream`, :mod:`fir_hip.crstream`): one :class:`Ext` per library, built from its name
and its EXPORTS table.  It loads ``libfir_<name>.so`` on first use, binds and checks the exports,
refuses a library built from other sources, and holds what the modules' ``route``,
``last_launch`` and host-array entries have in common.  Constructing one loads nothing.
"""
from __future__ import annotations

import ctypes
import threading
from pathlib import Path

import numpy as np

from . import FirHipError, _ptr, _share_torch_hip_runtime, _taps_cplx_i32

_HERE = Path(__file__).resolve().parent


class Ext:
    def __init__(self, name: str, exports: dict):
        self.name, self.exports = name, exports
        self._lib = None
        self._lock = threading.Lock()

    def lib_path(self) -> Path:
        return _HERE / f"libfir_{self.name}.so"

    def lib(self) -> ctypes.CDLL:
        """Load the library once; raise FirHipError if it is missing or built from other sources."""
        if self._lib is not None:
            return self._lib
        with self._lock:
            if self._lib is not None:
                return self._lib
            path = self.lib_path()
            if not path.exists():
                raise FirHipError(
                    f"{path} is not built: run `make -C warmup-fir-filter_amd/csrc_{self.name}` or "
                    "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
            _share_torch_hip_runtime()
            try:
                handle = ctypes.CDLL(str(path))
            except OSError as exc:
                raise FirHipError(f"cannot load {path}: {exc}") from exc
            for name, (res, args) in self.exports.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as exc:
                    raise FirHipError(f"{path} does not export {name}") from exc
                fn.restype = res
                fn.argtypes = args
            from ._srcid_ext import source_id

            built, want = getattr(handle, f"fir_{self.name}_build_id")().decode(), source_id(self.name)
            if want is not None and built != want:
                raise FirHipError(f"{path} was built from other sources (build id {built}, the sources beside it hash "
                                  f"to {want}): rebuild with `make -C warmup-fir-filter_amd/csrc_{self.name}`")
            self._lib = handle
        return self._lib

    def build_id(self) -> str:
        return getattr(self.lib(), f"fir_{self.name}_build_id")().decode()

    def last_error(self) -> str:
        return getattr(self.lib(), f"fir_{self.name}_last_error")().decode(errors="replace")

    def check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise FirHipError(f"{what} failed (status {rc}): {self.last_error()}")

    def route(self, entry: str, x_addr, y_addr, rows, width, hq, rates, frac_bits, acc_bits, out_stage) -> tuple[int, int]:
        """(route, bucket) of the library's ``entry`` (its fir_cplx_*_route) for these arguments;
        ``rates`` are the entry's rate arguments, in its order."""
        h = _taps_cplx_i32(hq)
        bucket = ctypes.c_int(0)
        r = getattr(self.lib(), entry)(int(x_addr), int(y_addr), int(rows), int(width), _ptr(h), h.shape[0],
                                       *(int(v) for v in rates), int(frac_bits), int(acc_bits), int(out_stage),
                                       ctypes.byref(bucket))
        if r < 0:
            raise FirHipError(f"{entry} refused the call: " + self.last_error())
        return r, bucket.value

    def route4(self, entry: str, addrs, rows, width, hq, rates, frac_bits, acc_bits, out_stage) -> tuple[int, int]:
        """:meth:`route` for an entry that takes four addresses (fir_cplx_stream_route, fir_cplx_rstream_route: x, hist_in, y
        and hist_out, 0 for NULL)."""
        h = _taps_cplx_i32(hq)
        bucket = ctypes.c_int(0)
        r = getattr(self.lib(), entry)(*(int(a) for a in addrs), int(rows), int(width), _ptr(h), h.shape[0],
                                       *(int(v) for v in rates), int(frac_bits), int(acc_bits), int(out_stage),
                                       ctypes.byref(bucket))
        if r < 0:
            raise FirHipError(f"{entry} refused the call: " + self.last_error())
        return r, bucket.value

    def last_launch(self, entry: str) -> tuple[int, int]:
        """(route, bucket) from the library's ``entry`` (its fir_cplx_*_last_launch)."""
        r, bucket = ctypes.c_int(0), ctypes.c_int(0)
        self.check(getattr(self.lib(), entry)(ctypes.byref(r), ctypes.byref(bucket)), entry)
        return r.value, bucket.value


def host_rows(x) -> tuple[np.ndarray, int, int]:
    """The host-array entries' view of x: x made contiguous, its rows and the values per row."""
    if not isinstance(x, np.ndarray) or x.dtype != np.int16:
        raise FirHipError(f"x must be an int16 array of interleaved (re, im), got {getattr(x, 'dtype', type(x).__name__)}")
    if x.ndim == 0:
        raise FirHipError("x must have at least one axis of interleaved (re, im) values")
    if x.shape[-1] % 2:
        raise FirHipError(f"x's last axis must hold an even number of values (re, im pairs), got {x.shape[-1]}")
    x = np.ascontiguousarray(x)
    rowlen = x.shape[-1]
    return x, (x.size // rowlen if rowlen else 0), rowlen
