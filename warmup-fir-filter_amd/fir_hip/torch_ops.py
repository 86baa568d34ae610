"""Device-tensor entry points of libfir_hip (torch tensors already resident in HBM).

PyTorch is plumbing here: it owns device memory, streams and ``torch.distributed``.
Every call enqueues the HIP kernel on the tensor's current stream through the C ABI
(``*_dev`` symbols of ``include/fir_hip.h``) and returns without synchronising.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import (IN_I16, IN_U8, MAX_TAPS, OUT_I32, OUT_U8_SAT, RESTORE_CLIP, RESTORE_NORMALIZE, FirHipError, _check,
               _taps2_f64, _taps_i32, decim_out_width, lib)

_IN = {torch.uint8: IN_U8, torch.int16: IN_I16}
_OUT_DTYPE = {OUT_U8_SAT: torch.uint8, OUT_I32: torch.int32}
# fixed-output dtypes of the metrics kernel (fir_num_dtype codes; bool = its 0/1 bytes)
_METRIC_DT = {torch.uint8: 0, torch.bool: 0, torch.int8: 1, torch.uint16: 2, torch.int16: 3, torch.uint32: 4,
              torch.int32: 5, torch.uint64: 6, torch.int64: 7, torch.float16: 8, torch.float32: 9, torch.float64: 10}


class Taps:
    """Quantized taps kept as a pinned-in-Python int32 array (no per-call conversion)."""

    def __init__(self, hq):
        self.h = _taps_i32(hq)
        self.ptr = self.h.ctypes.data_as(ctypes.c_void_p)
        self.n = int(self.h.size)


def _taps(hq) -> Taps:
    return hq if isinstance(hq, Taps) else Taps(hq)


def _stream_ptr(t: torch.Tensor, stream) -> ctypes.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream(t.device)
    return ctypes.c_void_p(s.cuda_stream)


def _check_dev(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise FirHipError(f"{name} must be a device tensor")
    if not t.is_contiguous():
        raise FirHipError(f"{name} must be contiguous")


def _check_out(out, shape, dtype, like, name: str = "out") -> None:
    """A caller's output: a contiguous device tensor of exactly ``shape`` and ``dtype`` on
    ``like``'s device.  The C entries take bare pointers, so this is the only size check between
    a torch caller and the kernel's stores."""
    _check_dev(out, name)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise FirHipError(f"{name} must be {dtype} of shape {tuple(shape)}, got {out.dtype} of shape "
                          f"{tuple(out.shape)}")
    if out.device != like.device:
        raise FirHipError(f"{name} must be on {like.device}, got {out.device}")


def _check_in(t, like, name: str) -> None:
    """A further input (a halo, the fixed array): a contiguous device tensor on ``like``'s device."""
    _check_dev(t, name)
    if t.device != like.device:
        raise FirHipError(f"{name} must be on {like.device}, got {t.device}")


def _check_work(work, need: int, like, what: str = "") -> None:
    """A caller's scratch buffer, checked by byte count (any dtype)."""
    if not work.is_cuda or not work.is_contiguous() or work.numel() * work.element_size() < need:
        raise FirHipError(f"work must be a contiguous device buffer of >= {need} bytes{what}")
    if work.device != like.device:
        raise FirHipError(f"work must be on {like.device}, got {work.device}")


def _no_overlap(inputs, outputs) -> None:
    """Refuse an output or work buffer whose bytes [data_ptr, data_ptr + numel * element_size)
    meet an input's or another output's on the same device (``inputs`` / ``outputs``: (name,
    tensor) pairs; empty tensors overlap nothing).  Every kernel reads a halo beyond the tile it
    writes, so nothing runs in place on the device."""
    spans = []
    for group in (inputs, outputs):
        spans.append([(n, t.device, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
                      for n, t in group if t.numel()])
    for k, (on, od, o0, o1) in enumerate(spans[1]):
        for n, d, p0, p1 in spans[0]:
            if d == od and o0 < p1 and p0 < o1:
                raise FirHipError(f"{on} must not overlap the input ({n})")
        for n, d, p0, p1 in spans[1][:k]:
            if d == od and o0 < p1 and p0 < o1:
                raise FirHipError(f"{on} must not overlap {n}")


def _out_dtype(out_stage: int):
    if out_stage not in _OUT_DTYPE:
        raise FirHipError(f"out_stage must be OUT_U8_SAT ({OUT_U8_SAT}) or OUT_I32 ({OUT_I32}), got {out_stage}")
    return _OUT_DTYPE[out_stage]


def _bank_i32(hq2):
    """(flat int32 taps, filters, taps per filter) of a (filters, taps) bank, each row through
    _taps_i32 as fir_hip.fir1d_fixed_rows_multi does (a plain int32 cast would wrap 2**31)."""
    h2 = np.asarray(hq2)
    if h2.ndim != 2 or h2.shape[0] < 1 or h2.shape[1] < 1:
        raise FirHipError("hq2 must be a non-empty (filters, taps) array")
    nf, L = h2.shape
    return np.concatenate([_taps_i32(row) for row in h2]), nf, L


def _rows_of(x, channels: int):
    """(rows, row length) of x's last axis, refusing a row that is no whole number of frames."""
    rowlen = x.shape[-1] if x.dim() else 1
    if channels < 1 or rowlen % channels:
        raise FirHipError("row length must be a multiple of channels")
    return (x.numel() // rowlen if rowlen else 0), rowlen


def fir1d_fixed_rows_dev(x: torch.Tensor, hq, frac_bits: int = 12, acc_bits: int = 32,
                         out_stage: int = OUT_I32, channels: int = 1, out: torch.Tensor | None = None,
                         stream=None) -> torch.Tensor:
    """Row-wise 1-D fixed FIR of a uint8/int16 device tensor (last axis = one row of
    width*channels interleaved samples)."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    t = _taps(hq)
    rows, rowlen = _rows_of(x, channels)
    if out is None:
        out = torch.empty(x.shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, x.shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir1d_fixed_rows_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], rows, rowlen // channels,
                                      channels, t.ptr, t.n, int(frac_bits), int(acc_bits), int(out_stage),
                                      ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir1d_fixed_rows_dev")
    return out


def fir1d_fixed_rows_decim_dev(x: torch.Tensor, hq, decim: int, phase: int = 0, frac_bits: int = 12,
                               acc_bits: int = 32, out_stage: int = OUT_I32, channels: int = 1,
                               out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """fir1d_fixed_rows_dev that keeps every ``decim``-th output frame from frame ``phase`` of each
    row (fir_decim_rows_dev): x's leading axes with a last axis of decim_out_width(width, decim,
    phase) * channels values.  One pass: x is read once and only the kept frames are written."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    t = _taps(hq)
    rows, rowlen = _rows_of(x, channels)
    ow = decim_out_width(rowlen // channels, decim, phase)
    shape = tuple(x.shape[:-1]) + (ow * channels,)
    if out is None:
        out = torch.empty(shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir_decim_rows_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], rows, rowlen // channels, channels,
                                    t.ptr, t.n, int(decim), int(phase), int(frac_bits), int(acc_bits), int(out_stage),
                                    ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)), "fir_decim_rows_dev")
    return out


def fir1d_fixed_rows_multi_dev(x: torch.Tensor, hq2, frac_bits: int = 12, acc_bits: int = 32,
                               out_stage: int = OUT_U8_SAT, channels: int = 1, out: torch.Tensor | None = None,
                               stream=None) -> torch.Tensor:
    """F filters (rows of hq2) over the same device tensor; returns (F, *x.shape)."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    h, nf, L = _bank_i32(hq2)
    rows, rowlen = _rows_of(x, channels)
    if out is None:
        out = torch.empty((nf,) + tuple(x.shape), dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, (nf,) + tuple(x.shape), _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    _check(lib().fir1d_fixed_rows_multi_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], rows, rowlen // channels,
                                            channels, h.ctypes.data_as(ctypes.c_void_p), L, nf, int(frac_bits),
                                            int(acc_bits), int(out_stage), ctypes.c_void_p(out.data_ptr()),
                                            _stream_ptr(x, stream)), "fir1d_fixed_rows_multi_dev")
    return out


class ImagesMultiPlan:
    """fir1d_fixed_images_multi_dev with its arguments checked and marshalled once: launch()
    re-issues the same call (the pipeline stage replayed on resident images) for the price of
    one C call.  outs[i] is either one (F, *xs[i].shape) tensor or a list of F tensors shaped like
    xs[i] (one buffer per output, as the reference keeps them; planes that start on 128 bytes
    store whole cache lines); allocated as (F, *shape) tensors when None."""

    def __init__(self, xs, hq2, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_U8_SAT,
                 channels: int = 1, outs=None):
        xs = list(xs)
        self._h, nf, L = _bank_i32(hq2)
        dt = _out_dtype(out_stage)
        if outs is None:
            outs = [torch.empty((nf,) + tuple(x.shape), dtype=dt, device=x.device) for x in xs]
        outs = list(outs)
        if len(outs) != len(xs):
            raise FirHipError("outs must hold one entry per image")
        planes, written = [], []
        for i, (x, o) in enumerate(zip(xs, outs)):
            _check_dev(x, f"xs[{i}]")
            if x.dtype not in _IN or x.dtype != xs[0].dtype:
                raise FirHipError(f"xs[{i}]: every image must be uint8, or every image int16")
            if x.device != xs[0].device:
                raise FirHipError(f"xs[{i}]: every image must be on {xs[0].device} (one launch, one device)")
            if channels < 1 or (x.shape[-1] if x.dim() else 1) % channels:
                raise FirHipError(f"xs[{i}]: row length must be a multiple of channels")
            if hasattr(o, "data_ptr"):  # one (F, *shape) tensor: plane f starts f planes in
                _check_out(o, (nf,) + tuple(x.shape), dt, xs[0], f"outs[{i}]")
                planes += [o.data_ptr() + f * x.numel() * o.element_size() for f in range(nf)]
                written.append((f"outs[{i}]", o))
                continue
            ps = list(o)
            if len(ps) != nf:
                raise FirHipError(f"outs[{i}] must hold {nf} planes shaped like xs[{i}] of the out_stage dtype")
            for f, p in enumerate(ps):
                _check_out(p, x.shape, dt, xs[0], f"outs[{i}][{f}]")
                planes.append(p.data_ptr())
                written.append((f"outs[{i}][{f}]", p))
        _no_overlap([(f"xs[{i}]", x) for i, x in enumerate(xs)], written)
        n = len(xs)
        rowlen = [x.shape[-1] if x.dim() else 1 for x in xs]
        self.xs, self.outs = xs, outs  # keep the buffers alive as long as the plan
        self._args = (n, (ctypes.c_void_p * max(n, 1))(*[x.data_ptr() for x in xs]),
                      (ctypes.c_int64 * max(n, 1))(*[x.numel() // r if r else 0 for x, r in zip(xs, rowlen)]),
                      (ctypes.c_int64 * max(n, 1))(*[r // channels for r in rowlen]),
                      _IN[xs[0].dtype] if xs else 0, channels, self._h.ctypes.data_as(ctypes.c_void_p), L, nf,
                      int(frac_bits), int(acc_bits), int(out_stage),
                      (ctypes.c_void_p * max(len(planes), 1))(*planes))
        self._fn = lib().fir1d_fixed_images_multi_dev

    def launch(self, stream=None):
        """Issue the call on `stream` (default: the current stream of the images' device)."""
        sp = _stream_ptr(self.xs[0], stream) if self.xs else None
        _check(self._fn(*self._args, sp), "fir1d_fixed_images_multi_dev")
        return self.outs


def fir1d_fixed_images_multi_dev(xs, hq2, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_U8_SAT,
                                 channels: int = 1, outs=None, stream=None) -> list:
    """The same F filters (rows of hq2) over several device images at once, outputs as
    ImagesMultiPlan describes; equal to fir1d_fixed_rows_dev per (image, filter), from one call
    (u8 -> sat-u8 banks: one launch per 8 images and 4 filters).  Replaces the per-image loop of
    fir_1d/sim/vector/gen_fixed_output.py:88-107 (reference root)."""
    return ImagesMultiPlan(xs, hq2, frac_bits, acc_bits, out_stage, channels, outs).launch(stream)


def _halo_ptrs(x: torch.Tensor, L: int, channels: int, halo_left, halo_right):
    """(ctypes pointers of the two halos, the (name, tensor) pairs among them): a halo is a device
    tensor of x's dtype on x's device, None, or an int address (the caller's responsibility)."""
    hl_n, hr_n = (L - 1 - L // 2) * channels, (L // 2) * channels
    ptrs, tensors = [], []
    for h, n, name in ((halo_left, hl_n, "halo_left"), (halo_right, hr_n, "halo_right")):
        if h is None or not n:
            ptrs.append(None)
        elif isinstance(h, int):
            ptrs.append(ctypes.c_void_p(h))
        else:
            _check_in(h, x, name)
            if h.dtype != x.dtype or h.numel() != n:
                raise FirHipError(f"{name} must hold {n} samples of {x.dtype}")
            ptrs.append(ctypes.c_void_p(h.data_ptr()))
            tensors.append((name, h))
    return ptrs, tensors


def _segment_args(x, hq, out, halo_left, halo_right, out_stage: int, channels: int):
    """The checks fir1d_fixed_edges_dev and fir1d_fixed_segment_dev share; (taps, halo pointers)."""
    t = _taps(hq)
    if channels < 1 or x.numel() % channels:
        raise FirHipError("segment length must be a multiple of channels")
    _check_out(out, x.shape, _out_dtype(out_stage), x)
    ptrs, halos = _halo_ptrs(x, t.n, channels, halo_left, halo_right)
    _no_overlap([("x", x)] + halos, [("out", out)])
    return t, ptrs


def fir1d_fixed_edges_dev(x: torch.Tensor, hq, out: torch.Tensor, halo_left, halo_right, frac_bits: int = 12,
                          acc_bits: int = 32, out_stage: int = OUT_I32, channels: int = 1, stream=None) -> torch.Tensor:
    """Recompute the halo-dependent edge outputs of a 1-D segment (see fir_hip.h) in ``out`` (of
    x's shape and the out_stage dtype, as fir1d_fixed_rows_dev filled it).  A halo is a
    device tensor of the segment's dtype, None (zeros), or an int device address holding the
    halo samples (e.g. a neighbour's HBM mapped by fir_hip.ipc_import: read over xGMI)."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    t, ptrs = _segment_args(x, hq, out, halo_left, halo_right, out_stage, channels)
    _check(lib().fir1d_fixed_edges_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], x.numel() // channels, channels,
                                       t.ptr, t.n, int(frac_bits), int(acc_bits), int(out_stage), ptrs[0], ptrs[1],
                                       ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir1d_fixed_edges_dev")
    return out


def fir1d_fixed_segment_dev(x: torch.Tensor, hq, halo_left, halo_right, frac_bits: int = 12, acc_bits: int = 32,
                            out_stage: int = OUT_I32, channels: int = 1, out: torch.Tensor | None = None,
                            stream=None) -> torch.Tensor:
    """One shard of a longer single-row signal with its halos (tensor, None = zeros, or an int
    device address such as a neighbour's mapped HBM): bulk + edges, one launch when possible."""
    _check_dev(x, "x")
    if x.dtype not in _IN:
        raise FirHipError(f"x dtype must be uint8 or int16, got {x.dtype}")
    if out is None:
        out = torch.empty(x.shape, dtype=_out_dtype(out_stage), device=x.device)
    t, (hl, hr) = _segment_args(x, hq, out, halo_left, halo_right, out_stage, channels)
    _check(lib().fir1d_fixed_segment_dev(ctypes.c_void_p(x.data_ptr()), _IN[x.dtype], x.numel() // channels,
                                         channels, t.ptr, t.n, int(frac_bits), int(acc_bits), int(out_stage), hl, hr,
                                         ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir1d_fixed_segment_dev")
    return out


def halo_mailbox_init_dev(mailbox: torch.Tensor, hl_bytes: int, hr_bytes: int, stream=None) -> torch.Tensor:
    """Zero a halo-gate mailbox (a 128-byte-aligned uint8 device tensor) with device atomics and
    record the halo sizes its slots are laid out for (every gate on it checks them)."""
    _check_dev(mailbox, "mailbox")
    _check(lib().fir_halo_mailbox_init_dev(ctypes.c_void_p(mailbox.data_ptr()), mailbox.numel() * mailbox.element_size(),
                                           int(hl_bytes), int(hr_bytes), _stream_ptr(mailbox, stream)),
           "fir_halo_mailbox_init_dev")
    return mailbox


def halo_gate_dev(seg: torch.Tensor, hl_bytes: int, hr_bytes: int, mailbox: torch.Tensor, left_mailbox: int | None,
                  right_mailbox: int | None, halo_left: torch.Tensor | None, halo_right: torch.Tensor | None,
                  status: torch.Tensor, timeout_s: float = 10.0, stream=None) -> None:
    """One step's ordered halo hand-off (fir_hip.h, fir_halo_gate_dev): publish this segment's
    edges, wait for both neighbours' (mapped mailbox addresses, None at a global end), copy
    theirs into ``halo_left`` / ``halo_right``; ``status`` (int32 device scalar) receives 0 or
    FIR_GATE_TIMEOUT."""
    _check_dev(seg, "seg")
    _check_dev(mailbox, "mailbox")
    for t, name in ((halo_left, "halo_left"), (halo_right, "halo_right"), (status, "status")):
        if t is not None:
            _check_dev(t, name)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _check(lib().fir_halo_gate_dev(ctypes.c_void_p(seg.data_ptr()), seg.numel() * seg.element_size(), int(hl_bytes),
                                   int(hr_bytes), ctypes.c_void_p(mailbox.data_ptr()),
                                   None if left_mailbox is None else ctypes.c_void_p(left_mailbox),
                                   None if right_mailbox is None else ctypes.c_void_p(right_mailbox),
                                   ptr(halo_left), ptr(halo_right), ptr(status), float(timeout_s),
                                   _stream_ptr(seg, stream)), "fir_halo_gate_dev")


def fir2d_fixed_dev(x: torch.Tensor, hq2, frac_bits: int = 12, acc_bits: int = 32, out_stage: int = OUT_U8_SAT,
                    out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """2-D fixed FIR of a uint8 device frame (H, W) or batch of frames (F, H, W), one launch."""
    _check_dev(x, "x")
    if x.dtype != torch.uint8 or x.dim() not in (2, 3):
        raise FirHipError("x must be a 2-D (frame) or 3-D (frames, height, width) uint8 device tensor")
    h2 = np.asarray(hq2.h if isinstance(hq2, Taps) else hq2)
    if h2.ndim != 2:
        raise FirHipError("hq2 must be 2-D")
    R, C = h2.shape
    t = Taps(h2.reshape(-1))
    if out is None:
        out = torch.empty(x.shape, dtype=_out_dtype(out_stage), device=x.device)
    _check_out(out, x.shape, _out_dtype(out_stage), x)
    _no_overlap([("x", x)], [("out", out)])
    frames = x.shape[0] if x.dim() == 3 else 1
    _check(lib().fir2d_fixed_frames_dev(ctypes.c_void_p(x.data_ptr()), frames, x.shape[-2], x.shape[-1], t.ptr, R, C,
                                        int(frac_bits), int(acc_bits), int(out_stage), ctypes.c_void_p(out.data_ptr()),
                                        _stream_ptr(x, stream)), "fir2d_fixed_frames_dev")
    return out


def fir2d_ideal_dev(x: torch.Tensor, h2, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """float64 ideal model of the 2-D FIR of a uint8 device frame (H, W) or batch of frames
    (F, H, W), one launch; the twin of fir2d_fixed_dev (see fir_hip.fir2d_ideal)."""
    _check_dev(x, "x")
    if x.dtype != torch.uint8 or x.dim() not in (2, 3):
        raise FirHipError("x must be a 2-D (frame) or 3-D (frames, height, width) uint8 device tensor")
    h = _taps2_f64(h2)
    R, C = h.shape
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    _check_out(out, x.shape, torch.float64, x)
    _no_overlap([("x", x)], [("out", out)])
    frames = x.shape[0] if x.dim() == 3 else 1
    _check(lib().fir2d_ideal_frames_dev(ctypes.c_void_p(x.data_ptr()), frames, x.shape[-2], x.shape[-1],
                                        h.ctypes.data_as(ctypes.c_void_p), R, C, ctypes.c_void_p(out.data_ptr()),
                                        _stream_ptr(x, stream)), "fir2d_ideal_frames_dev")
    return out


def fir1d_ideal_rows_dev(x: torch.Tensor, h, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """float64 ideal model over the uint8 rows (last axis) of a device tensor, into a float64
    tensor of x's shape (see fir_hip.fir1d_ideal_rows)."""
    _check_dev(x, "x")
    if x.dtype != torch.uint8:
        raise FirHipError("x must be uint8")
    hh = np.asarray(h)
    if hh.size == 0 or hh.size > MAX_TAPS:  # before any copy
        raise FirHipError(f"tap count must be in [1, {MAX_TAPS}]")
    hh = np.ascontiguousarray(np.asarray(hh, dtype=np.float64).reshape(-1))
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    _check_out(out, x.shape, torch.float64, x)
    _no_overlap([("x", x)], [("out", out)])
    width = x.shape[-1] if x.dim() else 1
    rows = x.numel() // width if width else 0
    _check(lib().fir1d_ideal_rows_dev(ctypes.c_void_p(x.data_ptr()), rows, width, hh.ctypes.data_as(ctypes.c_void_p),
                                      hh.size, ctypes.c_void_p(out.data_ptr()), _stream_ptr(x, stream)),
           "fir1d_ideal_rows_dev")
    return out


def restore_u8_dev(a: torch.Tensor, policy: int = RESTORE_CLIP, out: torch.Tensor | None = None,
                   work: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """f64 -> u8 restore conversion of a device tensor (restore_images.py:51-64)."""
    _check_dev(a, "a")
    if a.dtype != torch.float64:
        raise FirHipError("a must be float64")
    if out is None:
        out = torch.empty(a.shape, dtype=torch.uint8, device=a.device)
    _check_out(out, a.shape, torch.uint8, a)
    if policy == RESTORE_NORMALIZE and work is None:
        work = torch.empty(int(lib().fir_restore_work_bytes()), dtype=torch.uint8, device=a.device)
    elif work is not None:
        _check_work(work, int(lib().fir_restore_work_bytes()), a)
    _no_overlap([("a", a)], [("out", out)] + ([("work", work)] if work is not None else []))
    wp =ctypes.c_void_p(work.data_ptr()) if work is not None else None
    _check(lib().fir_restore_u8_dev(ctypes.c_void_p(a.data_ptr()), a.numel(), int(policy),
                                    ctypes.c_void_p(out.data_ptr()), wp, _stream_ptr(a, stream)), "fir_restore_u8_dev")
    return out


def compare_metrics_dev(ideal: torch.Tensor, fixed: torch.Tensor, out: torch.Tensor | None = None,
                        work: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """The 9 report sums of _compute_metrics (gen_3tap_compare_report.py:67-112) of device
    tensors, into a float64 device tensor of 9 (see fir_hip.metrics_from_sums)."""
    _check_dev(ideal, "ideal")
    _check_in(fixed, ideal, "fixed")
    if ideal.dtype != torch.float64 or fixed.dtype not in _METRIC_DT or ideal.shape != fixed.shape:
        raise FirHipError("ideal must be float64 and fixed an integer/bool/float tensor of the same shape")
    if out is None:
        out = torch.empty(9, dtype=torch.float64, device=ideal.device)
    _check_out(out, (9,), torch.float64, ideal)
    need = int(lib().fir_metrics_work_bytes(ideal.numel()))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=ideal.device)
    else:
        _check_work(work, need, ideal, f" for {ideal.numel()} samples")
    _no_overlap([("ideal", ideal), ("fixed", fixed)], [("out", out), ("work", work)])
    _check(lib().fir_compare_metrics_dev(ctypes.c_void_p(ideal.data_ptr()), ctypes.c_void_p(fixed.data_ptr()),
                                         _METRIC_DT[fixed.dtype], ideal.numel(), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(work.data_ptr()), _stream_ptr(ideal, stream)),
           "fir_compare_metrics_dev")
    return out
