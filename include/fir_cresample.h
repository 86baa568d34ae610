/* fir_cresample.h -- C ABI of libfir_cresample.so: the rational U/D resampling complex-tap 1-D
 * fixed-point FIR for complex int16 on the AMD Instinct MI355X (gfx950): zero-stuff by U, filter with
 * complex taps, keep every D-th output frame, in one pass (the last member of the rate-changing
 * family beside fir_cdecim.h's decimator and fir_cinterp.h's interpolator).
 *
 * An extension library beside libfir_hip.so, libfir_cdecim.so and libfir_cinterp.so: it shares
 * fir_hip.h's fir_status and fir_out_stage values and nothing else; no library loads or calls another.
 *
 * For up = U >= 1, decim = D >= 1, 0 <= phase < D:
 *
 *     mid_width   = width * U
 *     out_width   = mid_width > phase ? (mid_width - phase + D - 1) / D : 0
 *     y[r, m, :]  = y_up[r, m*D + phase, :]
 *
 * where y_up is exactly what fir_cplx_interp_rows (fir_cinterp.h) gives for the same hq, frac_bits,
 * acc_bits and out_stage; so: centre taps / 2, frames outside a row are zero, each of re and im one
 * exact integer sum wrapped once to acc_bits, round-half-up by frac_bits, the int32 or per-component
 * saturated-u8 stage; exact sums for acc_bits >= 64 (in 128 bits where the sum could pass 2^63).
 * x: rows x width frames of interleaved int16 (xr, xi).  hq: taps x 2 int32 (hr, hi) in HOST memory
 * (both forms).  y: C-contiguous rows x out_width x 2 values of the stage's type.  No conjugation
 * flag and no gain (unity passband gain needs the taps scaled by U).
 *
 * The kernels compute in polyphase form: with c0 = taps / 2, a_q = phase + c0 + q*D, p_q = a_q mod U
 * and c_q = a_q div U, output frame m = v*U + q (0 <= q < U) only meets the taps p_q + U*t, t >= 0,
 * p_q + U*t < taps, on the frames v*D + c_q - t:
 *
 *     re = sum_t hr[p_q + U*t] * xr[v*D + c_q - t] - hi[p_q + U*t] * xi[v*D + c_q - t]
 *     im = sum_t hr[p_q + U*t] * xi[v*D + c_q - t] + hi[p_q + U*t] * xr[v*D + c_q - t]
 *
 * A phase with p_q >= taps gives 0.  x is read once, no stuffed signal or intermediate is stored, no
 * tap meets a stuffed zero and no dropped frame is computed.
 *
 * Identities, all bit for bit and all of the arithmetic alone (nothing is forwarded across libraries):
 * decim = 1 is fir_cplx_interp_rows, up = 1 is fir_cplx_decim_rows (fir_cdecim.h), up = decim = 1 is
 * fir_cplx_rows (fir_hip.h), and taps whose every hi is 0 give fir_resample_rows(..., channels = 2)
 * with hr.  Calls with up = 1 or decim = 1 take the generic kernels here: use the dedicated, tuned
 * entries of fir_cdecim.h and fir_cinterp.h for them.
 *
 * Checks, in this order (fir_status; the text by fir_cresample_last_error):
 *   1. fir_cplx_rows_dev's: out_stage, rows and width, hq NULL, taps in [1, FIR_MAX_TAPS],
 *      frac_bits and acc_bits >= 1;
 *   2. "up must be >= 1", "decim must be >= 1", "phase must be in [0, decim)";
 *   3. the sizes: width * up, rows * out_width * 2 * 4 bytes and rows * width * 4 bytes must fit in
 *      int64;
 *   4. NULL x or y, only when the problem is not empty;
 *   5. only then, for the host form, the device: FIR_ENODEV for an index out of range or a device
 *      that is not gfx950.
 * Empty problems (rows = 0, width = 0, or out_width = 0 because mid_width <= phase) are no-ops
 * returning FIR_OK with route FIR_CRESAMPLE_NONE, NULL pointers and all.  No C++ exception crosses the
 * boundary.
 *
 * Dispatch.  One function decides the kernel from the checked arguments:
 *   FIR_CRESAMPLE_FAST        2 <= up <= 16, 2 <= decim <= 16, taps <= 128 with at most 32 taps per
 *                             phase (ceil(taps / up) <= 32), both parts of every tap in
 *                             [-32767, 32767], acc_bits <= 32, frac_bits <= 31, FIR_OUT_I32, x 16-byte
 *                             aligned, one row or rows of a multiple of 4 frames, and the grid fits
 *                             (width < 2^40, rows * ceil(out_width / (P * up)) < 2^31, P the periods
 *                             of a workgroup: 512 at decim = 2 or 3, else 256); y at any int32 address.
 *                             Taps travel by value in the kernel arguments, per output phase q two
 *                             packed tables in window order, zero-padded to the tap bucket, beside a
 *                             table of LDS offsets: nothing is allocated and no device table is read,
 *                             so the call can be captured in a hipGraph.
 *                             The tap bucket is the smallest of 1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24,
 *                             28, 32 that holds the longest sub-filter: max over q of n_q, n_q =
 *                             ceil((taps - p_q) / up) for p_q < taps, else 0 (bucket 1 when every
 *                             phase is empty).  The whole documented range is built: no instantiation
 *                             spills (profiles/cresample/resource_usage.txt) and the largest argument
 *                             block is 1.7 KiB.
 *   FIR_CRESAMPLE_GENERIC32   otherwise, when both parts of every tap are in [-32767, 32767],
 *                             acc_bits <= 32, frac_bits <= 31 and x is 4-byte aligned.
 *   FIR_CRESAMPLE_GENERIC128  otherwise, when acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768
 *                             could reach 2^63.
 *   FIR_CRESAMPLE_GENERIC64   every other legal call.
 * up = 1, decim = 1, up > 16 and decim > 16 take the generic kernels.  Those (one output frame per
 * thread, the interpolator's walk k = p_e, p_e + U, ... inside the row at j = m*D + phase) read their
 * taps from a device table that the library caches per device by the taps' bytes.  The FIRST use of a
 * table allocates and uploads it, which cannot be captured in a hipGraph: warm the call up once before
 * capturing.  A table first used inside a capture is kept for the life of the process.
 */
#ifndef FIR_CRESAMPLE_H
#define FIR_CRESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "fir_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The id of the sources the library was built from (fir_hip/_srcid_cresample.py recomputes it). */
const char* fir_cresample_build_id(void);

/* Text of the calling thread's last failure in this library (thread-local, as fir_last_error). */
const char* fir_cresample_last_error(void);

/* Frames a row of `width` frames has after resampling by up / decim at `phase` (the formula above);
 * -1 for up < 1, decim < 1, phase outside [0, decim), width < 0 or a width * up past int64. */
int64_t fir_cplx_resample_out_width(int64_t width, int up, int decim, int phase);

/* Host pointers; synchronous on `device`. */
int fir_cplx_resample_rows(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int taps,
                           int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y,
                           int device);

/* Device pointers; enqueues on `stream` (a hipStream_t, NULL: the default stream) of the current
 * device.  Never synchronises and does not detect an overlap of x and y. */
int fir_cplx_resample_rows_dev(const int16_t* x_dev, int64_t rows, int64_t width, const int32_t* hq, int taps,
                               int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage,
                               void* y_dev, void* stream);

enum { FIR_CRESAMPLE_NONE = 0, FIR_CRESAMPLE_FAST = 1, FIR_CRESAMPLE_GENERIC32 = 2, FIR_CRESAMPLE_GENERIC64 = 3,
       FIR_CRESAMPLE_GENERIC128 = 4 };

/* The route a call with these arguments would take (x_addr, y_addr: the addresses x and y would
 * have), without a device: FIR_CRESAMPLE_NONE for an empty problem, -1 for a call the checks refuse
 * (the text by fir_cresample_last_error).  *tap_bucket (may be NULL): the fast path's tap bucket,
 * 0 off the fast path. */
int fir_cplx_resample_route(uintptr_t x_addr, uintptr_t y_addr, int64_t rows, int64_t width, const int32_t* hq,
                            int taps, int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage,
                            int* tap_bucket);

/* What the calling thread's last fir_cplx_resample_rows[_dev] call that got past its checks actually
 * launched: *route (FIR_CRESAMPLE_NONE when it launched nothing, or before any call) and *tap_bucket
 * (either may be NULL).  Returns FIR_OK. */
int fir_cplx_resample_last_launch(int* route, int* tap_bucket);

#ifdef __cplusplus
}
#endif

#endif /* FIR_CRESAMPLE_H */
