/* fir_cstream.h -- C ABI of libfir_cstream.so: the streaming (block-continuous) decimating
 * complex-tap 1-D fixed-point FIR for complex int16 on the AMD Instinct MI355X (gfx950).
 *
 * An extension library beside libfir_hip.so: it shares fir_hip.h's fir_status and fir_out_stage
 * values and nothing else; neither library loads or calls the other, and it links against no other
 * library of the project.
 *
 * A caller filters and decimates one block of each row's stream, gives the history that precedes
 * the block, and gets back the history for the next block and the next phase.
 *
 *   x         rows x width frames of interleaved int16 (xr, xi), C-contiguous; every row is an
 *             independent stream.
 *   hq        taps x 2 int32 (hr, hi) in HOST memory (both forms).
 *   H         taps - 1.
 *   hist_in   rows x H frames, C-contiguous: the H frames that precede x in each row's stream,
 *             oldest first.  NULL: all zero (the start of a stream).
 *   phase     in [0, D): the index, inside this block, of the first kept frame.
 *
 * With X[r, i] = x[r, i] for 0 <= i < width and X[r, i] = hist_in[r, i + H] for -H <= i < 0:
 *
 *     s_re[r, n] = stage(round(wrap_acc( sum_k hr[k] * Xr[r, n-k] - hi[k] * Xi[r, n-k] )))   k in [0, taps)
 *     s_im[r, n] = stage(round(wrap_acc( sum_k hr[k] * Xi[r, n-k] + hi[k] * Xr[r, n-k] )))
 *     out_width      = width > phase ? ceil((width - phase) / D) : 0
 *     y[r, m, :]     = s[r, phase + m * D, :]                  m in [0, out_width)
 *     hist_out[r, j] = X[r, width - H + j]                     j in [0, H)
 *     next_phase     = phase + out_width * D - width           (always in [0, D))
 *
 * Causal: no centre shift and no zero padding on the right, so a block never needs a frame it has
 * not received.  wrap_acc, round, stage and the exactness rules are fir_cplx_rows' own (fir_hip.h):
 * each of re and im is one exact integer sum of its 2 * taps products wrapped once to acc_bits,
 * round-half-up by frac_bits, the int32 or per-component saturated-u8 stage; exact sums for
 * acc_bits >= 64 (in 128 bits where sum_k (|hr[k]| + |hi[k]|) * 32768 could reach 2^63).  No
 * conjugation and no gain.  y: C-contiguous rows x out_width x 2 values of the stage's type.
 *
 * The history output.  hist_out is the last H frames of hist_in ++ x; when width < H that mixes
 * both.  It must not overlap hist_in, x or y (the caller ping-pongs two history buffers).
 * hist_out = NULL: nothing is written.  With taps = 1 both history pointers are ignored.
 *
 * Empty problems.  rows = 0 is a no-op.  width = 0 with rows > 0 copies hist_in to hist_out (zeros
 * for a NULL hist_in).  out_width = 0 with width > 0 (phase >= width) writes only the history.
 *
 * Identities (tests/test_cstream_cases.py, tests/test_gpu_cstream.py):
 *   1. Split invariance.  For any widths w_1 .. w_B >= 0 that sum to N, run in turn with each
 *      block's hist_out and next_phase fed to the next, the outputs concatenate to the output of one
 *      block of N frames with the same initial history and phase; the final hist_out and next_phase
 *      are equal too.
 *   2. Against the one-shot entries.  With c = taps / 2 and Z = hist_in ++ x (H + width frames),
 *      s[n] = fir_cplx_rows(Z)[n + H - c]: y is frames [phase + H - c :: D][: out_width] of the
 *      full-rate complex-tap result over Z.  D = 1, zero history and hist_out = NULL is the causal
 *      form of fir_cplx_rows.
 *
 * Checks, in this order (fir_status; the text by fir_cstream_last_error):
 *   1. fir_cplx_rows_dev's: out_stage, rows and width, hq NULL, taps in [1, FIR_MAX_TAPS],
 *      frac_bits and acc_bits >= 1;
 *   2. "decim must be >= 1";
 *   3. "phase must be in [0, decim)";
 *   4. the sizes: rows * width * 2 * 4 bytes and rows * (taps - 1) * 4 bytes must fit in int64;
 *   5. NULL x when rows * width > 0, then NULL y when rows * out_width > 0;
 *   6. only then, for the host form, the device: FIR_ENODEV for an index out of range or a device
 *      that is not gfx950 (looked at only when something is computed or written).
 * No C++ exception crosses the boundary.
 *
 * Routes.  One function decides the FIR kernel from the checked arguments:
 *   FIR_CSTREAM_FAST        2 <= decim <= 16, taps <= 64, both parts of every tap in
 *                           [-32767, 32767], acc_bits <= 32, frac_bits <= 31, FIR_OUT_I32, x 16-byte
 *                           aligned, one row or rows of a multiple of 4 frames, both history
 *                           addresses 4-byte aligned (where they are given and H > 0), and the grid
 *                           fits (width < 2^40, rows * ceil(out_width / 512) < 2^31); y at any int32
 *                           address.  Taps travel by value in the kernel arguments, padded to the
 *                           tap bucket (the smallest of 2, 4, 6, 8, 12, 16, 24, 32, 48, 64 that
 *                           holds them): nothing is allocated and no device table is read, so a
 *                           block can be captured in a hipGraph.
 *   FIR_CSTREAM_GENERIC32   otherwise, when both parts of every tap are in [-32767, 32767],
 *                           acc_bits <= 32, frac_bits <= 31, x is 4-byte aligned and both histories
 *                           are 4-byte aligned (where they are given and H > 0).
 *   FIR_CSTREAM_GENERIC128  otherwise, when acc_bits >= 64 and sum_k (|hr[k]| + |hi[k]|) * 32768
 *                           could reach 2^63.
 *   FIR_CSTREAM_GENERIC64   every other legal call.
 * decim = 1 runs a generic route: a streaming full-rate filter on the sliding-window kernel of
 * fir_cplx_rows is a separate piece of work and out of scope here.
 * The generic kernels read their taps from a device table that the library caches per device by
 * the taps' bytes.  The FIRST use of a table allocates and uploads it, which cannot be captured
 * in a hipGraph: warm the call up once before capturing.
 * One small history kernel, the same on every route, writes hist_out on the same stream; it runs
 * when out_width = 0 and is skipped when hist_out is NULL or H = 0.
 */
#ifndef FIR_CSTREAM_H
#define FIR_CSTREAM_H

#include <stddef.h>
#include <stdint.h>

#include "fir_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The id of the sources the library was built from (fir_hip/_srcid_ext.py recomputes it). */
const char* fir_cstream_build_id(void);

/* Text of the calling thread's last failure in this library (thread-local, as fir_last_error). */
const char* fir_cstream_last_error(void);

/* Frames a block of `width` frames keeps; -1 for decim < 1, a phase outside [0, decim) or
 * width < 0 (as fir_cplx_decim_out_width). */
int64_t fir_cplx_stream_out_width(int64_t width, int decim, int phase);

/* The phase of the block that follows a block of `width` frames; -1 when invalid, as above. */
int fir_cplx_stream_next_phase(int64_t width, int decim, int phase);

/* Host pointers; synchronous on `device`. */
int fir_cplx_stream_block(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq,
                          int taps, int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y,
                          int16_t* hist_out, int device);

/* Device pointers; enqueues on `stream` (a hipStream_t, NULL: the default stream) of the current
 * device.  Never synchronises, never allocates on the fast route and detects no overlap. */
int fir_cplx_stream_block_dev(const int16_t* x_dev, const int16_t* hist_in_dev, int64_t rows, int64_t width,
                              const int32_t* hq, int taps, int decim, int phase, int frac_bits, int acc_bits,
                              int out_stage, void* y_dev, int16_t* hist_out_dev, void* stream);

enum { FIR_CSTREAM_NONE = 0, FIR_CSTREAM_FAST = 1, FIR_CSTREAM_GENERIC32 = 2, FIR_CSTREAM_GENERIC64 = 3,
       FIR_CSTREAM_GENERIC128 = 4 };

/* The route a call with these arguments would take (the four addresses x, hist_in, y and hist_out
 * would have; 0: NULL), without a device: FIR_CSTREAM_NONE when no FIR kernel runs (rows or
 * out_width equal to 0), -1 for a call the checks refuse (the text by fir_cstream_last_error).
 * *tap_bucket (may be NULL): the fast path's tap bucket, 0 off the fast path. */
int fir_cplx_stream_route(uintptr_t x_addr, uintptr_t hist_in_addr, uintptr_t y_addr, uintptr_t hist_out_addr,
                          int64_t rows, int64_t width, const int32_t* hq, int taps, int decim, int phase,
                          int frac_bits, int acc_bits, int out_stage, int* tap_bucket);

/* What the calling thread's last fir_cplx_stream_block[_dev] call that got past its checks launched
 * as its FIR kernel (the history kernel is not reported): *route (FIR_CSTREAM_NONE when it launched
 * none, or before any call) and *tap_bucket (either may be NULL).  Returns FIR_OK. */
int fir_cplx_stream_last_launch(int* route, int* tap_bucket);

#ifdef __cplusplus
}
#endif

#endif /* FIR_CSTREAM_H */
