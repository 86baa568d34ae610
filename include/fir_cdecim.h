/* fir_cdecim.h -- C ABI of libfir_cdecim.so: the decimating complex-tap 1-D fixed-point FIR for
 * complex int16 on the AMD Instinct MI355X (gfx950).
 *
 * An extension library beside libfir_hip.so: it shares fir_hip.h's fir_status and fir_out_stage
 * values and nothing else; neither library loads or calls the other.
 *
 * For decim = D >= 1 and 0 <= phase < D:
 *
 *     out_width  = width > phase ? (width - phase + D - 1) / D : 0
 *     y[r, m, :] = y_full[r, m * D + phase, :]        m in [0, out_width)
 *
 * with y_full exactly what fir_cplx_rows (fir_hip.h) gives for the same x, hq, frac_bits, acc_bits
 * and out_stage: centre taps / 2, frames outside a row are zero, each of re and im one exact integer
 * sum of its 2 * taps products wrapped once to acc_bits, round-half-up by frac_bits, the int32 or
 * per-component saturated-u8 stage; exact sums for acc_bits >= 64 (in 128 bits where the sum could
 * pass 2^63).  x: rows x width frames of interleaved int16 (xr, xi).  hq: taps x 2 int32 (hr, hi)
 * in HOST memory (both forms).  y: C-contiguous rows x out_width x 2 values of the stage's type.
 * No conjugation flag and no gain.  decim = 1 is fir_cplx_rows bit for bit; taps whose every hi is 0
 * give fir_decim_rows(..., channels = 2) with hr bit for bit (an identity of the arithmetic:
 * nothing is forwarded across libraries).  Skipped frames may be read; they influence nothing.
 *
 * Checks, in this order (fir_status; the text by fir_cdecim_last_error):
 *   1. fir_cplx_rows_dev's: out_stage, rows and width, hq NULL, taps in [1, FIR_MAX_TAPS],
 *      frac_bits and acc_bits >= 1;
 *   2. "decim must be >= 1";
 *   3. "phase must be in [0, decim)";
 *   4. the sizes: rows * width * 2 * 4 bytes must fit in int64;
 *   5. NULL x or y, only when the problem is not empty;
 *   6. only then, for the host form, the device: FIR_ENODEV for an index out of range or a device
 *      that is not gfx950.
 * Empty problems (rows, width or out_width equal to 0, which includes phase >= width) are no-ops
 * returning FIR_OK, NULL pointers and all.  No C++ exception crosses the boundary.
 *
 * Dispatch.  One function decides the kernel from the checked arguments:
 *   FIR_CDECIM_FAST        2 <= decim <= 16, taps <= 64, both parts of every tap in
 *                          [-32767, 32767], acc_bits <= 32, frac_bits <= 31, FIR_OUT_I32, x 16-byte
 *                          aligned, one row or rows of a multiple of 4 frames, and the grid fits
 *                          (width < 2^40, rows * ceil(out_width / 512) < 2^31); y at any int32
 *                          address.  Taps travel by value in the kernel arguments, padded to the
 *                          tap bucket (the smallest of 2, 4, 6, 8, 12, 16, 24, 32, 48, 64 that
 *                          holds them): nothing is allocated and no device table is read, so the
 *                          call can be captured in a hipGraph.
 *   FIR_CDECIM_GENERIC32   otherwise, when both parts of every tap are in [-32767, 32767],
 *                          acc_bits <= 32, frac_bits <= 31 and x is 4-byte aligned.
 *   FIR_CDECIM_GENERIC128  otherwise, when acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768
 *                          could reach 2^63.
 *   FIR_CDECIM_GENERIC64   every other legal call.
 * The generic kernels read their taps from a device table that the library caches per device by
 * the taps' bytes.  The FIRST use of a table allocates and uploads it, which cannot be captured
 * in a hipGraph: warm the call up once before capturing.  A table first used inside a capture is
 * kept for the life of the process.
 */
#ifndef FIR_CDECIM_H
#define FIR_CDECIM_H

#include <stddef.h>
#include <stdint.h>

#include "fir_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The id of the sources the library was built from (fir_hip/_srcid_cdecim.py recomputes it). */
const char* fir_cdecim_build_id(void);

/* Text of the calling thread's last failure in this library (thread-local, as fir_last_error). */
const char* fir_cdecim_last_error(void);

/* Frames a row of `width` frames keeps; -1 for decim < 1, a phase outside [0, decim) or width < 0. */
int64_t fir_cplx_decim_out_width(int64_t width, int decim, int phase);

/* Host pointers; synchronous on `device`. */
int fir_cplx_decim_rows(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int taps,
                        int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y, int device);

/* Device pointers; enqueues on `stream` (a hipStream_t, NULL: the default stream) of the current
 * device.  Never synchronises and does not detect an overlap of x and y. */
int fir_cplx_decim_rows_dev(const int16_t* x_dev, int64_t rows, int64_t width, const int32_t* hq, int taps,
                            int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y_dev,
                            void* stream);

enum { FIR_CDECIM_NONE = 0, FIR_CDECIM_FAST = 1, FIR_CDECIM_GENERIC32 = 2, FIR_CDECIM_GENERIC64 = 3,
       FIR_CDECIM_GENERIC128 = 4 };

/* The route a call with these arguments would take (x_addr, y_addr: the addresses x and y would
 * have), without a device: FIR_CDECIM_NONE for an empty problem, -1 for a call the checks refuse
 * (the text by fir_cdecim_last_error).  *tap_bucket (may be NULL): the fast path's tap bucket, 0 off
 * the fast path. */
int fir_cplx_decim_route(uintptr_t x_addr, uintptr_t y_addr, int64_t rows, int64_t width, const int32_t* hq,
                         int taps, int decim, int phase, int frac_bits, int acc_bits, int out_stage, int* tap_bucket);

/* What the calling thread's last fir_cplx_decim_rows[_dev] call that got past its checks actually
 * launched: *route (FIR_CDECIM_NONE when it launched nothing, or before any call) and *tap_bucket
 * (either may be NULL).  Returns FIR_OK. */
int fir_cplx_decim_last_launch(int* route, int* tap_bucket);

#ifdef __cplusplus
}
#endif

#endif /* FIR_CDECIM_H */
