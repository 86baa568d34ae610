"""NumPy checker of the float64 ideal 2-D FIR -- a test helper, not a test module.

The contract (include/fir_hip.h):

    y[i,j] = acc after:  acc = +0.0
                         for m in 0..R-1:            # outer, ascending
                           for n in 0..C-1:          # inner, ascending
                             acc = acc + h[m][n] * x[i - m + R//2][j - n + C//2]

with zero samples outside the frame.  ``ideal2d`` runs it vectorised over a zero-padded frame
(NumPy rounds the multiply and the add separately: two ufunc calls); ``ideal2d_loop`` is the
formula in plain Python floats, skipping the out-of-frame terms.  tests/test_ideal2d_ref.py proves
the two equal byte for byte, ties them to the reference's recorded 1-D outputs, and shows that the
checker sees a reordered sum.
"""
from __future__ import annotations

import numpy as np


def ideal2d(x, h, row_order=None) -> np.ndarray:
    """float64 (H, W) of a uint8 (H, W) frame under an (R, C) kernel.  ``row_order`` (a
    permutation of range(R)) sums the kernel rows in another order: only for the test that
    proves the order observable."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float64)
    if x.ndim != 2 or h.ndim != 2:
        raise ValueError("ideal2d takes a 2-D frame and a 2-D kernel")
    H, W = x.shape
    R, C = h.shape
    below, right = R // 2, C // 2  # rows below / columns right of an output that it reads
    above, left = R - 1 - below, C - 1 - right
    xp = np.zeros((H + R - 1, W + C - 1), np.float64)
    xp[above:above + H, left:left + W] = x
    acc = np.zeros((H, W), np.float64)
    for m in (range(R) if row_order is None else row_order):
        for n in range(C):
            # x[i - m + R//2][j - n + C//2] = xp[i + (R-1-m)][j + (C-1-n)]
            acc = acc + h[m, n] * xp[R - 1 - m:R - 1 - m + H, C - 1 - n:C - 1 - n + W]
    return acc


def ideal2d_loop(x, h) -> np.ndarray:
    """The formula as written, in Python floats (IEEE double, one rounding per operation)."""
    x = np.asarray(x)
    H, W = x.shape
    hh = [[float(v) for v in row] for row in np.asarray(h, dtype=np.float64).tolist()]
    R, C = len(hh), len(hh[0])
    xs = [[float(v) for v in row] for row in x.tolist()]
    y = np.zeros((H, W), np.float64)
    for i in range(H):
        for j in range(W):
            acc = 0.0
            for m in range(R):
                ii = i - m + R // 2
                if ii < 0 or ii >= H:
                    continue
                for n in range(C):
                    jj = j - n + C // 2
                    if jj < 0 or jj >= W:
                        continue
                    acc = acc + hh[m][n] * xs[ii][jj]
            y[i, j] = acc
    return y
