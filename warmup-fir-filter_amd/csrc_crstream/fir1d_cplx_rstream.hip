// fir1d_cplx_rstream.hip — the streaming (block-continuous) rational U/D resampling complex-tap 1-D
// fixed-point FIR for complex int16: zero-stuff one block of each row's stream by U, filter it behind
// the history that precedes it, keep every D-th frame, and write the history of the next block.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); H = (L - 1) / U
//   X[r, i] = x[r, i] for 0 <= i < width, hist_in[r, i + H] for -H <= i < 0 (0 for a NULL hist_in)
//   out_width = width * U > phase ? (width * U - phase + D - 1) / D : 0
//   j = m * D + phase, e = j mod U, i = j div U; the taps e + U*t < L:
//   re[m] = stage(round(wrap_acc( sum_t hr[e+U*t] * Xr[i-t] - hi[e+U*t] * Xi[i-t] )))
//   im[m] = stage(round(wrap_acc( sum_t hr[e+U*t] * Xi[i-t] + hi[e+U*t] * Xr[i-t] )))
//   hist_out[r, j] = X[r, width - H + j]
//
// The arithmetic is csrc/fir1d_cplx.hip's (one exact sum per part, wrapped once, overflow-free
// round-half-up, int32 or saturated-u8 stage), causal: no centre shift, nothing read past the block.
// This file is libfir_crstream.so's own device side; it shares the header-only device helpers of
// csrc/ (fir_common.h, fir_dispatch.h) and of csrc_cext/ (cext_device.h) and nothing compiled from
// either.
//
//  * fir1d_cplx_rstream_kernel — the hot path (FIR_CRSTREAM_FAST, see route_of): cext_device.h's
//    resampling tile kernel, the one-shot resampler's (csrc_cresample/fir1d_cplx_resample.hip
//    describes the work split, the D input planes, the tables and the output stage), with two
//    differences.  The plan is causal: a_q = phase + q * D (no + L / 2), p_q = a_q mod U,
//    c_q = a_q div U, n_q = ceil((L - p_q) / U); output frame m = v * U + q meets the taps
//    p_q + U * t at the frames v * D + c_q - t.  c_q >= 0 and n_q - 1 <= (L - 1) / U = H, so the
//    lowest window start S = min_q (c_q - n_q + 1) is >= -H; c_q <= D - 1 and n_q >= need - 1
//    (need: the longest n_q), so a window's first dword k0_q = c_q - n_q + 1 - S is <= D, inside
//    the offset table.  And the row's history is one more argument: of a 16-byte chunk that is not
//    wholly inside [0, width), a frame f with -H <= f < 0 is read from hist_in[r, H + f] (zero for a
//    NULL history), a frame f < -H or f >= width is zero.  A workgroup's first window starts at
//    v0 * D + S >= -H, so only the up to 3 frames of the 16-byte lead lie below -H.  A bucket's
//    zero-padded tail may fall past width: those frames are staged as zero and meet zero taps.
//
//  * The generic kernels — every other legal call (up or decim of 1 or above 16 among them): one
//    kept output frame per thread, walking t = 0 .. (L - 1 - e) / U over the frames i - t (>= -H
//    always) with the read switched to the history below frame 0; with a NULL history the walk
//    stops at frame 0.  Taps from a cached device table.
//    fir1d_cplx_rstream_generic32_kernel: 32-bit wrap-around sums, two v_dot2 per tap.
//    fir1d_cplx_rstream_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
//
//  * fir1d_cplx_rstream_hist_kernel — one thread per (row, j) writes hist_out[r, j] from
//    x[r, width - H + j] when that index is >= 0, else from hist_in[r, width + j] (zero for NULL).
//    The same on every route, on the same stream, after the FIR kernel (no dependence: hist_out
//    overlaps nothing).  It runs when out_width = 0; skipped for a NULL hist_out or H = 0.
#include <string>

#include "cext_launch.h"
#include "crstream.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace crstream {

using cext::kChunk;  // frames per staging step of one thread (16 bytes)
using cext::launch_recorded;
using fir::kBlock;
using fir::OutTraits;

// cext::ResampleTaps under this library's own name (its kernels' symbols carry it)
template <int NP>
struct TapsRs : cext::ResampleTaps<NP> {};

// hist: the first frame of hist_in (rows x H frames), or NULL for a zero history
template <int NP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_rstream_kernel(const uint32_t* __restrict__ x,
                                                                    const uint32_t* __restrict__ hist,
                                                                    int32_t* __restrict__ y, int64_t width,
                                                                    int64_t out_width, uint32_t groups, int U, int D,
                                                                    int P, int T, int S, int ext, int H, int PL,
                                                                    uint32_t magic, TapsRs<NP> taps, int shl, int frac) {
    cext::resample_tile<NP, ACC32, true>(x, hist, y, width, out_width, groups, U, D, P, T, S, ext, H, PL, magic, taps, shl,
                                         frac);
}

// One kept output frame per thread: frame gi = r * out_width + m is intermediate frame
// j = m * D + phase = i * U + e of row r's stream and sums the taps e + U * t over the frames i - t
// (>= -H for every t; below 0: the history, and with a NULL history the walk stops at frame 0);
// taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_rstream_generic_kernel(
    const int16_t* __restrict__ x, const int16_t* __restrict__ hist, typename OutTraits<STAGE>::T* __restrict__ y,
    int64_t n_out, int64_t width, int64_t out_width, int64_t U, int64_t D, int64_t phase, int64_t H,
    const int32_t* __restrict__ taps, int L, int frac, int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t j = m * D + phase;  // < width * U
    const int64_t i = j / U, e = j % U;
    const int64_t t_max = e < L ? (L - 1 - e) / U : -1;  // <= H
    const int64_t t_hi = hist || i >= t_max ? t_max : i;
    const int16_t* __restrict__ xr = x + 2 * r * width;
    const int16_t* __restrict__ hr_ = hist ? hist + 2 * (r * H + H) : nullptr;  // frame f < 0 at hr_[2 f]
    cext::Acc<WIDE> re = 0, im = 0;
    for (int64_t t = 0; t <= t_hi; ++t) cext::cmac<WIDE>(re, im, taps, e + U * t, i - t >= 0 ? xr : hr_, i - t);
    cext::store_frame<STAGE, WIDE>(y, gi, re, im, frac, acc_bits);
}

// The same walk on 32-bit wrap-around accumulators over the packed table; a frame is one aligned
// dword, of x or of the history.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_rstream_generic32_kernel(
    const uint32_t* __restrict__ x, const uint32_t* __restrict__ hist, typename OutTraits<STAGE>::T* __restrict__ y,
    int64_t n_out, int64_t width, int64_t out_width, int64_t U, int64_t D, int64_t phase, int64_t H,
    const uint32_t* __restrict__ pk, int L, int shl, int frac) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t j = m * D + phase;
    const int64_t i = j / U, e = j % U;
    const int64_t t_max = e < L ? (L - 1 - e) / U : -1;
    const int64_t t_x = i < t_max ? i : t_max;             // taps 0..t_x meet x, the rest the history
    const uint32_t* __restrict__ xf = x + r * width + i;  // tap e + U * t meets frame xf[-t] while i - t >= 0
    uint32_t re = 0, im = 0;
    for (int64_t t = 0; t <= t_x; ++t) cext::cmac32(re, im, pk, e + U * t, xf[-t]);
    if (hist) {
        const uint32_t* __restrict__ hf = hist + r * H + H + i;  // frame i - t < 0 at hf[-t]
        for (int64_t t = t_x + 1; t <= t_max; ++t) cext::cmac32(re, im, pk, e + U * t, hf[-t]);
    }
    cext::store_frame32<STAGE>(y, gi, re, im, shl, frac);
}

// hist_out[r, j] = X[r, width - H + j]: FrameT is uint32_t when all three arrays are 4-byte
// aligned (a frame is one dword), else a pair of int16.
struct rs_frame16 {
    int16_t re, im;
};
template <typename FrameT>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_rstream_hist_kernel(const FrameT* __restrict__ x,
                                                                         const FrameT* __restrict__ hist_in,
                                                                         FrameT* __restrict__ hist_out, int64_t n_hist,
                                                                         int64_t width, int64_t H) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_hist) return;
    const int64_t j = gi % H, r = gi / H;
    const int64_t f = width - H + j;  // the frame of the block; below 0: frame H + f = width + j of hist_in
    FrameT v{};
    if (f >= 0)
        v = x[r * width + f];
    else if (hist_in)
        v = hist_in[r * H + width + j];
    hist_out[gi] = v;
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t out_width(int64_t width, int up, int decim, int phase) {
    int64_t mid = 0;
    if (width < 0 || up < 1 || decim < 1 || phase < 0 || phase >= decim || __builtin_mul_overflow(width, (int64_t)up, &mid))
        return -1;
    return mid > phase ? (mid - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

int next_phase(int64_t width, int up, int decim, int phase) {
    int64_t mid = 0;
    if (width < 0 || up < 1 || decim < 1 || phase < 0 || phase >= decim || __builtin_mul_overflow(width, (int64_t)up, &mid))
        return -1;
    if (mid <= phase) return (int)(phase - mid);
    // mid - phase = q * D + rem + 1 and out_width = q + 1: out_width * D - (mid - phase) = D - 1 - rem
    return decim - 1 - (int)((mid - phase - 1) % decim);
}

int hist_frames(int L, int up) { return L < 1 || up < 1 ? -1 : (L - 1) / up; }

// cext::check_head (csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its
// order and its texts), then the header's checks 2 to 4.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int decim,
          int phase, int frac, int acc_bits, int stage, int64_t* ow, std::string* err) {
    if (const int rc = cext::check_head(rows, width, hq, L, frac, acc_bits, stage, err)) return rc;
    if (up < 1) return *err = "up must be >= 1", FIR_EINVAL;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    *ow = out_width(width, up, decim, phase);
    int64_t ro = 0, rw = 0, rh = 0;
    if (*ow < 0 || __builtin_mul_overflow(rows, *ow, &ro) || ro > INT64_MAX / 8 || __builtin_mul_overflow(rows, width, &rw) ||
        rw > INT64_MAX / 4)
        return *err = "width * up, rows * out_width * 2 * 4 bytes and rows * width * 4 bytes must fit in int64", FIR_EINVAL;
    if (__builtin_mul_overflow(rows, (int64_t)hist_frames(L, up), &rh) || rh > INT64_MAX / 4)
        return *err = "rows * ((taps - 1) / up) * 4 bytes must fit in int64", FIR_EINVAL;
    if (rw != 0 && !x) return *err = "x and y must not be NULL", FIR_EINVAL;
    if (ro != 0 && !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    return FIR_OK;
}

int route_of(uintptr_t x, uintptr_t hist_in, uintptr_t y, uintptr_t hist_out, int64_t rows, int64_t width, int64_t ow,
             const int32_t* hq, int L, int up, int decim, int phase, int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    // a frame of a history is one dword to the 32-bit kernels (NULL and H = 0: no history is read)
    const bool h4 = hist_frames(L, up) == 0 || (hist_in % 4 == 0 && hist_out % 4 == 0);
    if (d2 && h4 && up >= 2 && up <= cext::kRsMaxUD && decim >= 2 && decim <= cext::kRsMaxUD && L <= cext::kRsMaxTaps &&
        (L + up - 1) / up <= cext::kRsMaxNP && stage == FIR_OUT_I32 && x % 16 == 0 &&
        (rows == 1 || width % kChunk == 0)) {  // every row starts as x does
        const int64_t per = (int64_t)cext::rs_periods(decim) * up;  // output frames per workgroup
        const int64_t groups = (ow + per - 1) / per;
        // the grid is rows * groups < 2^31 workgroups; the kernel holds a group index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / groups) {
            *bucket = cext::rs_bucket_of(cext::rs_plan_of(L, up, decim, phase, 0).need);
            return FIR_CRSTREAM_FAST;
        }
    }
    if (d2 && h4 && x % 4 == 0) return FIR_CRSTREAM_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CRSTREAM_GENERIC128 : FIR_CRSTREAM_GENERIC64;
}

// what the calling thread's last launch() launched as its FIR kernel: those go through
// cext::launch_recorded, the history kernel does not
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

static hipError_t launch_fast(int bucket, const void* x, const void* hist, void* y, int64_t rows, int64_t width,
                              int64_t ow, const int32_t* hq, int L, int U, int D, int phase, int frac, int acc_bits,
                              hipStream_t s) {
    const cext::RsPlan pl = cext::rs_plan_of(L, U, D, phase, 0);  // causal
    const int H = hist_frames(L, U);
    return cext::with_rs_bucket(bucket, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        cext::RsGeom g;
        TapsRs<NP> t = {};
        // never taken: S >= -H and k0 <= D by the plan, the rest as in the one-shot resampler
        if (pl.S < -H || !cext::rs_setup<NP>(hq, U, D, pl, rows, ow, &g, &t)) return hipErrorInvalidValue;
        if (acc_bits == 32)
            return launch_recorded(FIR_CRSTREAM_FAST, NP, fir1d_cplx_rstream_kernel<NP, true>, g.grid, g.lds, s,
                                   (const uint32_t*)x, (const uint32_t*)hist, (int32_t*)y, width, ow, g.groups, U, D, g.P,
                                   g.T, pl.S, g.ext, H, g.PL, g.magic, t, 0, frac);
        return launch_recorded(FIR_CRSTREAM_FAST, NP, fir1d_cplx_rstream_kernel<NP, false>, g.grid, g.lds, s,
                               (const uint32_t*)x, (const uint32_t*)hist, (int32_t*)y, width, ow, g.groups, U, D, g.P, g.T,
                               pl.S, g.ext, H, g.PL, g.magic, t, 32 - acc_bits, frac);
    });
}

// the history kernel: not recorded (last_launch reports the FIR kernel)
static hipError_t launch_hist(const int16_t* x, const int16_t* hist_in, int16_t* hist_out, int64_t rows, int64_t width,
                              int64_t H, hipStream_t s) {
    const int64_t n_hist = rows * H;
    const int64_t blocks = (n_hist + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (((uintptr_t)x | (uintptr_t)hist_in | (uintptr_t)hist_out) % 4 == 0)
        hipLaunchKernelGGL(fir1d_cplx_rstream_hist_kernel<uint32_t>, grid, dim3(kBlock), 0, s, (const uint32_t*)x,
                           (const uint32_t*)hist_in, (uint32_t*)hist_out, n_hist, width, H);
    else
        hipLaunchKernelGGL(fir1d_cplx_rstream_hist_kernel<rs_frame16>, grid, dim3(kBlock), 0, s, (const rs_frame16*)x,
                           (const rs_frame16*)hist_in, (rs_frame16*)hist_out, n_hist, width, H);
    return hipGetLastError();
}

int launch(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq, int L, int up,
           int decim, int phase, int frac, int acc_bits, int stage, void* y, int16_t* hist_out, hipStream_t stream,
           std::string* err) {
    int64_t ow = 0;
    const int rc = check(x, y, rows, width, hq, L, up, decim, phase, frac, acc_bits, stage, &ow, err);
    if (rc) return rc;
    cext::launch_none();
    if (rows == 0) return FIR_OK;
    const int H = hist_frames(L, up);
    if (H == 0) hist_in = nullptr, hist_out = nullptr;  // no history: both pointers are ignored
    if (ow != 0) {
        int bucket = 0;
        const int route = route_of((uintptr_t)x, (uintptr_t)hist_in, (uintptr_t)y, (uintptr_t)hist_out, rows, width, ow,
                                   hq, L, up, decim, phase, frac, acc_bits, stage, &bucket);
        hipError_t e;
        if (route == FIR_CRSTREAM_FAST)
            e = launch_fast(bucket, x, hist_in, y, rows, width, ow, hq, L, up, decim, phase, frac, acc_bits, stream);
        else
            e = fir::with_stage(stage, [&](auto st) {
                return cext::launch_generic(
                    route, FIR_CRSTREAM_GENERIC32, FIR_CRSTREAM_GENERIC128, fir1d_cplx_rstream_generic32_kernel<st>,
                    fir1d_cplx_rstream_generic_kernel<st, false>, fir1d_cplx_rstream_generic_kernel<st, true>, rows * ow,
                    hq, L, frac, acc_bits, stream, [&](auto kernel, dim3 grid, const void* table, int t0, int t1) {
                        return launch_recorded(route, 0, kernel, grid, 0, stream, x, hist_in, y, rows * ow, width, ow,
                                               (int64_t)up, (int64_t)decim, (int64_t)phase, (int64_t)H, table, L, t0, t1);
                    });
            });
        if (e != hipSuccess)
            return *err = std::string("fir1d cplx rstream launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    }
    if (hist_out) {
        const hipError_t e = launch_hist(x, hist_in, hist_out, rows, width, H, stream);
        if (e != hipSuccess)
            return *err = std::string("fir1d cplx rstream history launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    }
    return FIR_OK;
}

}  // namespace crstream
