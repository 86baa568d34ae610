/* fir_cinterp.h -- C ABI of libfir_cinterp.so: the interpolating complex-tap 1-D fixed-point FIR for
 * complex int16 on the AMD Instinct MI355X (gfx950): zero-stuff by U, then filter with complex taps
 * (the digital up-converter beside fir_cdecim.h's down-converter).
 *
 * An extension library beside libfir_hip.so and libfir_cdecim.so: it shares fir_hip.h's fir_status
 * and fir_out_stage values and nothing else; no library loads or calls another.
 *
 * For up = U >= 1:
 *
 *     out_width      = width * U
 *     xu[r, i*U, :]  = x[r, i, :], every other frame of xu is zero       (rows x out_width frames)
 *     y              = exactly what fir_cplx_rows (fir_hip.h) gives for xu with the same hq,
 *                      frac_bits, acc_bits and out_stage
 *
 * so: centre taps / 2, frames outside a row are zero, each of re and im one exact integer sum
 * wrapped once to acc_bits, round-half-up by frac_bits, the int32 or per-component saturated-u8
 * stage; exact sums for acc_bits >= 64 (in 128 bits where the sum could pass 2^63).  x: rows x width
 * frames of interleaved int16 (xr, xi).  hq: taps x 2 int32 (hr, hi) in HOST memory (both forms).
 * y: C-contiguous rows x out_width x 2 values of the stage's type.  No conjugation flag and no gain
 * (unity passband gain needs the taps scaled by U).  The row keeps the U - 1 stuffed frames after its
 * last input frame.  up = 1 is fir_cplx_rows bit for bit; taps whose every hi is 0 give
 * fir_interp_rows(..., channels = 2) with hr bit for bit (an identity of the arithmetic: nothing is
 * forwarded across libraries).
 *
 * The kernels compute in polyphase form: with c0 = taps / 2, output frame i*U + e (0 <= e < U) only
 * meets the taps p_e + U*t, p_e = (e + c0) mod U, c_e = (e + c0) div U, t >= 0, p_e + U*t < taps:
 *
 *     re = sum_t hr[p_e + U*t] * xr[i + c_e - t] - hi[p_e + U*t] * xi[i + c_e - t]
 *     im = sum_t hr[p_e + U*t] * xi[i + c_e - t] + hi[p_e + U*t] * xr[i + c_e - t]
 *
 * x is read once, no stuffed signal is stored and no tap meets a stuffed zero.
 *
 * Checks, in this order (fir_status; the text by fir_cinterp_last_error):
 *   1. fir_cplx_rows_dev's: out_stage, rows and width, hq NULL, taps in [1, FIR_MAX_TAPS],
 *      frac_bits and acc_bits >= 1;
 *   2. "up must be >= 1";
 *   3. the sizes: rows * width * up * 2 * 4 bytes must fit in int64;
 *   4. NULL x or y, only when the problem is not empty;
 *   5. only then, for the host form, the device: FIR_ENODEV for an index out of range or a device
 *      that is not gfx950.
 * Empty problems (rows or width equal to 0) are no-ops returning FIR_OK, NULL pointers and all.  No
 * C++ exception crosses the boundary.
 *
 * Dispatch.  One function decides the kernel from the checked arguments:
 *   FIR_CINTERP_FAST        2 <= up <= 16, taps <= 128 with at most 32 taps per phase
 *                           (ceil(taps / up) <= 32), both parts of every tap in [-32767, 32767],
 *                           acc_bits <= 32, frac_bits <= 31, FIR_OUT_I32, x 16-byte aligned, one row
 *                           or rows of a multiple of 4 frames, and the grid fits (width < 2^40,
 *                           rows * ceil(width / 2048) < 2^31); y at any int32 address.  Taps travel
 *                           by value in the kernel arguments, per phase two packed tables in window
 *                           order, zero-padded to the window bucket: nothing is allocated and no
 *                           device table is read, so the call can be captured in a hipGraph.
 *                           The window bucket is the smallest of 1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24,
 *                           28, 33 that holds the window all phases share: W = hi - lo + 1 input
 *                           frames, lo the least c_e - n_e + 1 and hi the greatest c_e over the phases
 *                           with n_e > 0 taps (n_e = ceil((taps - p_e) / up) for p_e < taps, else 0).
 *                           W is ceil(taps / up) or one more.  The whole documented range is built:
 *                           no instantiation spills (profiles/cinterp/resource_usage.txt) and the
 *                           largest argument block is 1.5 KiB.
 *   FIR_CINTERP_GENERIC32   otherwise, when both parts of every tap are in [-32767, 32767],
 *                           acc_bits <= 32, frac_bits <= 31 and x is 4-byte aligned.
 *   FIR_CINTERP_GENERIC128  otherwise, when acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768
 *                           could reach 2^63.
 *   FIR_CINTERP_GENERIC64   every other legal call, up = 1 and up > 16 included.
 * The generic kernels (one output frame per thread, walking k = p_e, p_e + U, ... inside the row)
 * read their taps from a device table that the library caches per device by the taps' bytes.  The
 * FIRST use of a table allocates and uploads it, which cannot be captured in a hipGraph: warm the
 * call up once before capturing.  A table first used inside a capture is kept for the life of the
 * process.
 */
#ifndef FIR_CINTERP_H
#define FIR_CINTERP_H

#include <stddef.h>
#include <stdint.h>

#include "fir_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The id of the sources the library was built from (fir_hip/_srcid_cinterp.py recomputes it). */
const char* fir_cinterp_build_id(void);

/* Text of the calling thread's last failure in this library (thread-local, as fir_last_error). */
const char* fir_cinterp_last_error(void);

/* Frames a row of `width` frames has after zero-stuffing: width * up; -1 for up < 1, width < 0 or a
 * product past int64. */
int64_t fir_cplx_interp_out_width(int64_t width, int up);

/* Host pointers; synchronous on `device`. */
int fir_cplx_interp_rows(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int taps,
                         int up, int frac_bits, int acc_bits, int out_stage, void* y, int device);

/* Device pointers; enqueues on `stream` (a hipStream_t, NULL: the default stream) of the current
 * device.  Never synchronises and does not detect an overlap of x and y. */
int fir_cplx_interp_rows_dev(const int16_t* x_dev, int64_t rows, int64_t width, const int32_t* hq, int taps,
                             int up, int frac_bits, int acc_bits, int out_stage, void* y_dev, void* stream);

enum { FIR_CINTERP_NONE = 0, FIR_CINTERP_FAST = 1, FIR_CINTERP_GENERIC32 = 2, FIR_CINTERP_GENERIC64 = 3,
       FIR_CINTERP_GENERIC128 = 4 };

/* The route a call with these arguments would take (x_addr, y_addr: the addresses x and y would
 * have), without a device: FIR_CINTERP_NONE for an empty problem, -1 for a call the checks refuse
 * (the text by fir_cinterp_last_error).  *window_bucket (may be NULL): the fast path's window bucket,
 * 0 off the fast path. */
int fir_cplx_interp_route(uintptr_t x_addr, uintptr_t y_addr, int64_t rows, int64_t width, const int32_t* hq,
                          int taps, int up, int frac_bits, int acc_bits, int out_stage, int* window_bucket);

/* What the calling thread's last fir_cplx_interp_rows[_dev] call that got past its checks actually
 * launched: *route (FIR_CINTERP_NONE when it launched nothing, or before any call) and
 * *window_bucket (either may be NULL).  Returns FIR_OK. */
int fir_cplx_interp_last_launch(int* route, int* window_bucket);

#ifdef __cplusplus
}
#endif

#endif /* FIR_CINTERP_H */
