"""The reference of the complex-tap FIR (fir_cplx_rows) -- a test helper, not a test module.

The committed C oracle has no complex-tap form, but it pins this arithmetic through an identity.
View a row of ``width`` complex int16 frames as a real one-channel signal of ``2 * width`` samples
(s[2f] = xr[f], s[2f+1] = xi[f]).  With c = taps // 2 and G = 4c + 3, two real tap sets of length G
(centre G // 2 = 2c + 1)

    g_re[2k] = -hi[k]   g_re[2k+1] = hr[k]
    g_im[2k+1] = hr[k]  g_im[2k+2] = hi[k]

give, at the even samples of the first and the odd samples of the second, exactly the two sums of
the contract (include/fir_hip.h): output sample 2n of g_re meets s[2n - j + 2c + 1], i.e. for
j = 2k + 1 the sample 2(n - k + c) = xr[n-k+c] with hr[k], and for j = 2k the sample
2(n - k + c) + 1 = xi[n-k+c] with -hi[k]; likewise 2n + 1 of g_im.  The zero padding of the real
row at both ends is the zero padding of whole frames, the wrap, rounding and stage are the
oracle's own, each applied once to one exact integer sum:

    re = oracle.fir1d_rows(x, g_re, frac, acc, stage, channels=1)[..., 0::2]
    im = oracle.fir1d_rows(x, g_im, frac, acc, stage, channels=1)[..., 1::2]

``want`` computes that through ``c_oracle()``; ``cplx_loop`` is the contract itself as a direct
Python-int loop (unbounded ints, so exact for every tap size and acc_bits), for small inputs:
tests/test_cplx_ref.py holds the first against the second before anything leans on it.  The C
oracle sums in 64 bits: exact mod 2^64 for acc_bits < 64, and for acc_bits >= 64 while the true
sum stays below 2^63; a case past that is compared with ``cplx_loop`` alone.
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle

OUT_U8_SAT, OUT_I32 = 0, 1


def as_real_taps(hq):
    """(g_re, g_im): the two real tap sets of length 4 * (taps // 2) + 3, as int64 arrays."""
    h = np.asarray(hq, dtype=np.int64).reshape(-1, 2)
    L = h.shape[0]
    G = 4 * (L // 2) + 3
    g_re, g_im = np.zeros(G, np.int64), np.zeros(G, np.int64)
    for k in range(L):
        g_re[2 * k] = -h[k, 1]
        g_re[2 * k + 1] = h[k, 0]
        g_im[2 * k + 1] = h[k, 0]
        g_im[2 * k + 2] = h[k, 1]
    return g_re, g_im


def want(x, hq, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    """What fir_cplx_rows must give for the int16 array x (last axis 2 * width interleaved values)."""
    x = np.ascontiguousarray(x, dtype=np.int16)
    y = np.zeros(x.shape, np.uint8 if stage == OUT_U8_SAT else np.int32)
    if x.size == 0:
        return y
    g_re, g_im = as_real_taps(hq)
    # -hi of an int32-sized hi = -2^31 does not fit the oracle's int32 taps
    assert g_re.min() >= -(1 << 31) and g_re.max() < (1 << 31), "a tap part of -2^31 has no int32 negation"
    o = c_oracle()
    y[..., 0::2] = o.fir1d_rows(x, g_re, frac, acc, stage, channels=1)[..., 0::2]
    y[..., 1::2] = o.fir1d_rows(x, g_im, frac, acc, stage, channels=1)[..., 1::2]
    return y


def cplx_loop(x, hq, frac: int = 12, acc: int = 32, stage: int = OUT_I32) -> np.ndarray:
    """The contract as plain Python ints, row by row and frame by frame (small inputs only)."""
    x = np.asarray(x, dtype=np.int16)
    h = [(int(a), int(b)) for a, b in np.asarray(hq, dtype=object).reshape(-1, 2)]
    L, c = len(h), len(h) // 2
    x2 = x.reshape(-1, x.shape[-1])
    width = x2.shape[1] // 2
    mask, sign, bias = (1 << acc) - 1, 1 << (acc - 1), 1 << (frac - 1)

    def finish(v: int) -> int:
        v &= mask
        if v & sign:
            v -= 1 << acc
        v = (v + bias) >> frac
        if stage == OUT_U8_SAT:
            return 0 if v < 0 else (255 if v > 255 else v)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the int32 stage keeps the low 32 bits

    out = np.zeros(x2.shape, np.uint8 if stage == OUT_U8_SAT else np.int32)
    for r in range(x2.shape[0]):
        row = [int(v) for v in x2[r]]
        for n in range(width):
            re = im = 0
            for k in range(L):
                f = n - k + c
                if 0 <= f < width:
                    xr, xi = row[2 * f], row[2 * f + 1]
                    re += h[k][0] * xr - h[k][1] * xi
                    im += h[k][0] * xi + h[k][1] * xr
            out[r, 2 * n], out[r, 2 * n + 1] = finish(re), finish(im)
    return out.reshape(x.shape)
