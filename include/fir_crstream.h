/* fir_crstream.h -- C ABI of libfir_crstream.so: the streaming (block-continuous) rational U/D
 * resampling complex-tap 1-D fixed-point FIR for complex int16 on the AMD Instinct MI355X (gfx950).
 *
 * An extension library beside libfir_hip.so: it shares fir_hip.h's fir_status and fir_out_stage
 * values and nothing else; neither library loads or calls the other, and it links against no other
 * library of the project.
 *
 * A caller resamples one block of each row's stream by U / D (zero-stuff by U, filter, keep every
 * D-th frame), gives the history that precedes the block, and gets back the history for the next
 * block and the next phase.
 *
 *   x         rows x width frames of interleaved int16 (xr, xi), C-contiguous; every row is an
 *             independent stream.
 *   hq        taps x 2 int32 (hr, hi) in HOST memory (both forms).  L = taps, U = up, D = decim.
 *   H         (L - 1) div U (integer division): fir_cplx_rstream_hist_frames(taps, up).
 *   hist_in   rows x H frames, C-contiguous: the H frames that precede x in each row's stream,
 *             oldest first.  NULL: all zero (the start of a stream).
 *   phase     in [0, D): the index, in the block's width * U intermediate frames, of the first kept
 *             frame.
 *
 * With X[r, i] = x[r, i] for 0 <= i < width and X[r, i] = hist_in[r, i + H] for -H <= i < 0, the
 * intermediate frame j has e = j mod U and i = j div U:
 *
 *     s_re[r, j] = stage(round(wrap_acc( sum_t hr[e+U*t] * Xr[r, i-t] - hi[e+U*t] * Xi[r, i-t] )))   t >= 0, e + U*t < L
 *     s_im[r, j] = stage(round(wrap_acc( sum_t hr[e+U*t] * Xi[r, i-t] + hi[e+U*t] * Xr[r, i-t] )))
 *     mid_width      = width * U
 *     out_width      = mid_width > phase ? ceil((mid_width - phase) / D) : 0
 *     y[r, m, :]     = s[r, phase + m * D, :]                  m in [0, out_width)
 *     hist_out[r, j] = X[r, width - H + j]                     j in [0, H)
 *     next_phase     = phase + out_width * D - mid_width       (always in [0, D))
 *
 * Causal: no centre shift and nothing is read past the block; t <= (L - 1 - e) div U <= H, so
 * i - t >= -H always holds.  wrap_acc, round, stage and the exactness rules are
 * fir_cplx_resample_rows' own (fir_cresample.h): each of re and im is one exact integer sum wrapped
 * once to acc_bits, round-half-up by frac_bits, the int32 or per-component saturated-u8 stage; exact
 * sums for acc_bits >= 64 (in 128 bits where sum_k (|hr[k]| + |hi[k]|) * 32768 could reach 2^63).
 * No conjugation and no gain.  y: C-contiguous rows x out_width x 2 values of the stage's type.
 *
 * The history output.  hist_out is the last H frames of hist_in ++ x; when width < H that mixes
 * both.  It must not overlap hist_in, x or y (the caller ping-pongs two history buffers).
 * hist_out = NULL: nothing is written.  With H = 0 (taps <= up) both history pointers are ignored.
 *
 * Empty problems.  rows = 0 is a no-op.  width = 0 with rows > 0 copies hist_in to hist_out (zeros
 * for a NULL hist_in).  out_width = 0 with width > 0 (phase >= width * up) writes only the history.
 *
 * Identities (tests/test_crstream_cases.py, tests/test_gpu_crstream.py):
 *   1. Split invariance.  For any widths w_1 .. w_B >= 0 that sum to N, run in turn with each
 *      block's hist_out and next_phase fed to the next, the outputs concatenate to the output of one
 *      block of N frames with the same initial history and phase; the final hist_out and next_phase
 *      are equal too.
 *   2. Against the one-shot entries.  With c0 = L / 2 and Z = one zero frame ++ hist_in ++ x
 *      (1 + H + width frames), s[j] = fir_cplx_interp_rows(Z)[j + (H + 1) * U - c0]: y is frames
 *      [phase + (H + 1) * U - c0 :: D][: out_width] of the one-shot interpolator over Z.  The zero
 *      frame is there because H * U can be below c0 (L = 3, U = 4: H = 0, c0 = 1); with it the
 *      offset is never negative ((H + 1) * U >= L > c0), and no frame past the end of Z is read.
 *   3. up = 1 is fir_cplx_stream_block (fir_cstream.h), bit for bit: y, hist_out and next_phase,
 *      and H = L - 1 there.
 *
 * Checks, in this order (fir_status; the text by fir_crstream_last_error):
 *   1. fir_cplx_rows_dev's: out_stage, rows and width, hq NULL, taps in [1, FIR_MAX_TAPS],
 *      frac_bits and acc_bits >= 1;
 *   2. "up must be >= 1", "decim must be >= 1", "phase must be in [0, decim)";
 *   3. the sizes: width * up, rows * out_width * 2 * 4 bytes and rows * width * 4 bytes, then
 *      rows * H * 4 bytes, must fit in int64;
 *   4. NULL x when rows * width > 0, then NULL y when rows * out_width > 0;
 *   5. only then, for the host form, the device: FIR_ENODEV for an index out of range or a device
 *      that is not gfx950 (looked at only when something is computed or written).
 * No C++ exception crosses the boundary.
 *
 * Routes.  One function decides the FIR kernel from the checked arguments:
 *   FIR_CRSTREAM_FAST        fir_cresample.h's conditions: 2 <= up <= 16 and 2 <= decim <= 16, taps
 *                            <= 128 and at most 32 per phase (ceil(taps / up) <= 32), both parts of
 *                            every tap in [-32767, 32767], acc_bits <= 32, frac_bits <= 31,
 *                            FIR_OUT_I32, x 16-byte aligned, one row or rows of a multiple of 4
 *                            frames, and the grid fits (width < 2^40, rows * ceil(out_width /
 *                            (P * up)) < 2^31 with P = 512 periods per workgroup at decim = 2 or 3,
 *                            else 256); plus both history addresses 4-byte aligned (where they are
 *                            given and H > 0); y at any int32 address.  The kernel is
 *                            fir_cplx_resample_rows' with a causal plan: with a_q = phase + q * D,
 *                            p_q = a_q mod U, c_q = a_q div U, output frame m = v * U + q meets the
 *                            taps p_q + U * t, t in [0, n_q), n_q = ceil((L - p_q) / U) (0 for
 *                            p_q >= L), at the frames v * D + c_q - t.  Taps travel by value in the
 *                            kernel arguments, padded per phase to the tap bucket (the smallest of
 *                            1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32 that holds the longest
 *                            n_q; 1 when every phase is empty): nothing is allocated and no device
 *                            table is read, so a block can be captured in a hipGraph.
 *   FIR_CRSTREAM_GENERIC32   otherwise, when both parts of every tap are in [-32767, 32767],
 *                            acc_bits <= 32, frac_bits <= 31, x is 4-byte aligned and both histories
 *                            are 4-byte aligned (where they are given and H > 0).
 *   FIR_CRSTREAM_GENERIC128  otherwise, when acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768
 *                            could reach 2^63.
 *   FIR_CRSTREAM_GENERIC64   every other legal call.
 * up = 1, decim = 1, up > 16 and decim > 16 run a generic route.  For up = 1 the tuned path is
 * fir_cplx_stream_block (fir_cstream.h), which gives the same values; a tuned streaming
 * interpolator (decim = 1) is out of scope here.
 * The generic kernels read their taps from a device table that the library caches per device by
 * the taps' bytes.  The FIRST use of a table allocates and uploads it, which cannot be captured
 * in a hipGraph: warm the call up once before capturing.
 * One small history kernel, the same on every route, writes hist_out on the same stream; it runs
 * when out_width = 0 and is skipped when hist_out is NULL or H = 0.
 */
#ifndef FIR_CRSTREAM_H
#define FIR_CRSTREAM_H

#include <stddef.h>
#include <stdint.h>

#include "fir_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The id of the sources the library was built from (fir_hip/_srcid_ext.py recomputes it). */
const char* fir_crstream_build_id(void);

/* Text of the calling thread's last failure in this library (thread-local, as fir_last_error). */
const char* fir_crstream_last_error(void);

/* Frames a block of `width` frames keeps; -1 for up < 1, decim < 1, a phase outside [0, decim),
 * width < 0 or a width * up past int64 (as fir_cplx_resample_out_width). */
int64_t fir_cplx_rstream_out_width(int64_t width, int up, int decim, int phase);

/* The phase of the block that follows a block of `width` frames; -1 when invalid, as above. */
int fir_cplx_rstream_next_phase(int64_t width, int up, int decim, int phase);

/* H, the frames of history per row: (taps - 1) div up; -1 for taps < 1 or up < 1. */
int fir_cplx_rstream_hist_frames(int taps, int up);

/* Host pointers; synchronous on `device`. */
int fir_cplx_rstream_block(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq,
                           int taps, int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y,
                           int16_t* hist_out, int device);

/* Device pointers; enqueues on `stream` (a hipStream_t, NULL: the default stream) of the current
 * device.  Never synchronises, never allocates on the fast route and detects no overlap. */
int fir_cplx_rstream_block_dev(const int16_t* x_dev, const int16_t* hist_in_dev, int64_t rows, int64_t width,
                               const int32_t* hq, int taps, int up, int decim, int phase, int frac_bits, int acc_bits,
                               int out_stage, void* y_dev, int16_t* hist_out_dev, void* stream);

enum { FIR_CRSTREAM_NONE = 0, FIR_CRSTREAM_FAST = 1, FIR_CRSTREAM_GENERIC32 = 2, FIR_CRSTREAM_GENERIC64 = 3,
       FIR_CRSTREAM_GENERIC128 = 4 };

/* The route a call with these arguments would take (the four addresses x, hist_in, y and hist_out
 * would have; 0: NULL), without a device: FIR_CRSTREAM_NONE when no FIR kernel runs (rows or
 * out_width equal to 0), -1 for a call the checks refuse (the text by fir_crstream_last_error).
 * *tap_bucket (may be NULL): the fast path's tap bucket, 0 off the fast path. */
int fir_cplx_rstream_route(uintptr_t x_addr, uintptr_t hist_in_addr, uintptr_t y_addr, uintptr_t hist_out_addr,
                           int64_t rows, int64_t width, const int32_t* hq, int taps, int up, int decim, int phase,
                           int frac_bits, int acc_bits, int out_stage, int* tap_bucket);

/* What the calling thread's last fir_cplx_rstream_block[_dev] call that got past its checks launched
 * as its FIR kernel (the history kernel is not reported): *route (FIR_CRSTREAM_NONE when it launched
 * none, or before any call) and *tap_bucket (either may be NULL).  Returns FIR_OK. */
int fir_cplx_rstream_last_launch(int* route, int* tap_bucket);

#ifdef __cplusplus
}
#endif

#endif /* FIR_CRSTREAM_H */
