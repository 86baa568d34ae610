"""2-D FIR models: float64 ideal, fixed-point, and their comparison.

The reference has no 2-D model (its ``fir_2d`` tree is empty); the assignment it was written for
defines the 2-D result as "float sum, round, clip to [0, 255]".  This module is the 2-D twin of
``fir_1d/model/python/fir_1d_ref.py`` / ``fir_1d_fixed_ref.py``: the same validators (so the
error texts are the reference's), the same host-side quantization, and the sums on the GPU
(``fir2d_ideal`` / ``fir2d_fixed`` in libfir_hip.so).  There is no CPU fallback.

Arithmetic (include/fir_hip.h): ``y[i, j] = sum over m, then n (both ascending) of
h[m][n] * x[i - m + R//2][j - n + C//2]``, zero outside the frame; the ideal model rounds every
product and sum on its own in float64 and does not clamp, the fixed model quantizes h to
Q(coeff_bits - frac_bits).frac_bits, wraps the exact sum to ``acc_bits``, rounds half up by
``frac_bits`` and saturates to uint8 (fir_1d_fixed_ref.py:95-126).

Order of checks (each model stops at the first that fails):
  1. h is a non-empty rectangular R x C sequence of numbers;
  2. ``_validate_h_coefficients`` on h flattened row-major (the index reported is the flat one);
  3. x has two dimensions, and is prepared row by row by ``_prepare_rows_u8`` (finite check,
     round half up, clamp, uint8);
  4. fixed model only: ``_coeff_stage`` on the flattened h (bit widths, Q range, quantization).
An empty frame returns an empty array without a device call.
"""
from __future__ import annotations

import numpy as np
import numpy.typing as npt

import fir_hip
from fir_1d.model.python.fir_1d_fixed_ref import _coeff_stage, device_bits
from fir_1d.model.python.fir_1d_ref import _prepare_rows_u8, _validate_h_coefficients

_BAD_H = "Invalid h: h must be a non-empty 2-D array of coefficients."
_BAD_X = "Invalid x: x must be a 2-D array of samples (height, width)."


def _kernel_rows(h) -> tuple[int, int, list]:
    """(R, C, h flattened row-major) of a rectangular kernel; ValueError otherwise."""
    if isinstance(h, (str, bytes)):
        raise ValueError(_BAD_H)
    try:
        rows = [list(r) for r in h]
    except TypeError:  # a scalar, or a 1-D sequence (its elements do not iterate)
        raise ValueError(_BAD_H) from None
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError(_BAD_H)
    flat = [v for r in rows for v in r]
    if any(np.ndim(v) != 0 for v in flat):  # three or more dimensions
        raise ValueError(_BAD_H)
    return len(rows), len(rows[0]), flat


def _frame_u8(x) -> np.ndarray:
    a = x if isinstance(x, np.ndarray) else np.asarray(x)
    if a.ndim != 2:
        raise ValueError(_BAD_X)
    return _prepare_rows_u8(a)


def fir_2d_ideal(x, h) -> npt.NDArray[np.float64]:
    """float64 ideal 2-D FIR of an (H, W) frame with an (R, C) kernel: float64 (H, W), no clamp."""
    R, C, flat = _kernel_rows(h)
    _validate_h_coefficients(flat)
    x_u8 = _frame_u8(x)
    if x_u8.size == 0:
        return np.zeros(x_u8.shape, dtype=np.float64)
    return fir_hip.fir2d_ideal(x_u8, np.array([float(v) for v in flat], dtype=np.float64).reshape(R, C))


def fir_2d_fixed_golden(x, h, frac_bits: int = 12, acc_bits: int = 32,
                        coeff_bits: int = 16) -> npt.NDArray[np.uint8]:
    """Fixed-point 2-D FIR of an (H, W) frame: uint8 (H, W), the hardware-behaviour model."""
    R, C, flat = _kernel_rows(h)
    _validate_h_coefficients(flat)
    x_u8 = _frame_u8(x)
    hq = _coeff_stage(flat, frac_bits, acc_bits, coeff_bits)
    if x_u8.size == 0:
        return np.zeros(x_u8.shape, dtype=np.uint8)
    f, a = device_bits(frac_bits, acc_bits)
    return fir_hip.fir2d_fixed(x_u8, hq.reshape(R, C), f, a, fir_hip.OUT_U8_SAT)


def fir_2d_compare(x, h, frac_bits: int = 12, acc_bits: int = 32, coeff_bits: int = 16) -> dict:
    """The fixed-vs-ideal report of one frame: ``fir_hip.compare_metrics(ideal, fixed)`` with the
    report's keys (num_samples, max_abs_err, mae, rmse, mean_err, sat_low_ratio, sat_high_ratio,
    sat_ratio, clip_needed_ratio)."""
    R, C, flat = _kernel_rows(h)
    _validate_h_coefficients(flat)
    x_u8 = _frame_u8(x)
    hq = _coeff_stage(flat, frac_bits, acc_bits, coeff_bits)
    if x_u8.size == 0:
        return fir_hip.metrics_from_sums(np.zeros(9), 0)
    f, a = device_bits(frac_bits, acc_bits)
    ideal = fir_hip.fir2d_ideal(x_u8, np.array([float(v) for v in flat], dtype=np.float64).reshape(R, C))
    fixed = fir_hip.fir2d_fixed(x_u8, hq.reshape(R, C), f, a, fir_hip.OUT_U8_SAT)
    return fir_hip.compare_metrics(ideal, fixed)
