// fir1d_cplx_stream.hip — the streaming (block-continuous) decimating complex-tap 1-D fixed-point
// FIR for complex int16: filter and decimate one block of each row's stream behind the history that
// precedes it, and write the history of the next block.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); H = L - 1
//   X[r, i] = x[r, i] for 0 <= i < width, hist_in[r, i + H] for -H <= i < 0 (0 for a NULL hist_in)
//   out_width = width > phase ? (width - phase + D - 1) / D : 0;   n = m * D + phase
//   re[m] = stage(round(wrap_acc( sum_k hr[k] * Xr[n-k] - hi[k] * Xi[n-k] )))
//   im[m] = stage(round(wrap_acc( sum_k hr[k] * Xi[n-k] + hi[k] * Xr[n-k] )))
//   hist_out[r, j] = X[r, width - H + j]
//
// The arithmetic is csrc/fir1d_cplx.hip's (one exact sum per part, wrapped once, overflow-free
// round-half-up, int32 or saturated-u8 stage), causal: no centre shift, nothing read past the block.
// This file is libfir_cstream.so's own device side; it shares the header-only device helpers of
// csrc/ (fir_common.h, fir_dispatch.h) and of csrc_cext/ (cext_device.h) and nothing compiled from
// either.
//
//  * fir1d_cplx_stream_kernel — the hot path (FIR_CSTREAM_FAST, see route_of): cext_device.h's
//    decimating tile kernel (its comment describes the tiling, the D LDS planes, the magic division
//    and the stepped MAC loop) with a causal window origin, base = phase - (L - 1), and the row's
//    history as one more argument.  Of a 16-byte chunk that is not wholly inside [0, width), a frame
//    f with -H <= f < 0 is read from hist_in[r, H + f] (zero for a NULL history), a frame f < -H or
//    f >= width is zero.  A workgroup's first window starts at m0 * D + base >= -H, so only the up
//    to 3 frames of the 16-byte lead lie below -H.  The window's zero-padded far end (LP - L frames
//    past n) may fall past width: those frames are staged as zero and meet zero taps.
//
//  * The generic kernels — every other legal call: one kept output frame per thread, walking all
//    L taps (n - k >= -H always holds) with the read switched to the history below frame 0; with a
//    NULL history the walk stops at frame 0.  Taps from a cached device table.
//    fir1d_cplx_stream_generic32_kernel: 32-bit wrap-around sums, two v_dot2 per tap, and a
//    wave-uniform untested loop for workgroups whose windows all lie inside the block.
//    fir1d_cplx_stream_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
//
//  * fir1d_cplx_stream_hist_kernel — one thread per (row, j) writes hist_out[r, j] from
//    x[r, width - H + j] when that index is >= 0, else from hist_in[r, width + j] (zero for NULL).
//    The same on every route, on the same stream, after the FIR kernel (no dependence: hist_out
//    overlaps nothing).  It runs when out_width = 0; skipped for a NULL hist_out or H = 0.
#include <string>

#include "cext_launch.h"
#include "cstream.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cstream {

using cext::launch_recorded;
using fir::kBlock;
using fir::OutTraits;

// cext::TileTaps under the name the kernel's signature, and so its symbol, has always carried
template <int LP>
struct TapsCs : cext::TileTaps<LP> {};

// hist: the first frame of hist_in (rows x H frames), or NULL for a zero history
template <int LP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_stream_kernel(const uint32_t* __restrict__ x,
                                                                   const uint32_t* __restrict__ hist,
                                                                   int32_t* __restrict__ y, int64_t width,
                                                                   int64_t out_width, uint32_t groups, int G, int D,
                                                                   int base, int H, int PL, uint32_t magic,
                                                                   TapsCs<LP> taps, int shl, int frac) {
    cext::decim_tile<LP, ACC32, true>(x, hist, y, width, out_width, groups, G, D, base, H, PL, magic, taps, shl, frac);
}

// One kept output frame per thread: frame gi = r * out_width + m sums tap k over frame
// n - k = m * D + phase - k of row r's stream (>= -H for every k; below 0: the history, and with a
// NULL history the walk stops at frame 0); taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_stream_generic_kernel(
    const int16_t* __restrict__ x, const int16_t* __restrict__ hist, typename OutTraits<STAGE>::T* __restrict__ y,
    int64_t n_out, int64_t width, int64_t out_width, int64_t D, int64_t phase, const int32_t* __restrict__ taps, int L,
    int frac, int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t n = m * D + phase;  // tap k reads frame n - k; n < width
    const int64_t H = L - 1;
    const int64_t k_hi = hist || n >= H ? H : n;
    const int16_t* __restrict__ xr = x + 2 * r * width;
    const int16_t* __restrict__ hr_ = hist ? hist + 2 * (r * H + H) : nullptr;  // frame f < 0 at hr_[2 f]
    cext::Acc<WIDE> re = 0, im = 0;
    for (int64_t k = 0; k <= k_hi; ++k) cext::cmac<WIDE>(re, im, taps, k, n - k >= 0 ? xr : hr_, n - k);
    cext::store_frame<STAGE, WIDE>(y, gi, re, im, frac, acc_bits);
}

// The same walk on 32-bit wrap-around accumulators over the packed table; a frame is one aligned
// dword, of x or of the history.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_stream_generic32_kernel(
    const uint32_t* __restrict__ x, const uint32_t* __restrict__ hist, typename OutTraits<STAGE>::T* __restrict__ y,
    int64_t n_out, int64_t width, int64_t out_width, int64_t D, int64_t phase, const uint32_t* __restrict__ pk, int L,
    int shl, int frac) {
    const int64_t b0 = (int64_t)blockIdx.x * kBlock;
    const int64_t gi = b0 + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t n = m * D + phase;
    const int64_t H = L - 1;
    const uint32_t* __restrict__ xf = x + r * width + n;  // tap k meets frame xf[-k] while n - k >= 0
    uint32_t re = 0, im = 0;
    // A workgroup whose 256 outputs lie in one row, with every window inside the block (known from
    // its first output, so the same for every lane), walks all L taps without a test: the loop is
    // wave-uniform and its taps come by scalar loads.  At a block's start each lane takes the
    // frames below 0 from the history.
    const int64_t bm = b0 % out_width;
    if (bm + kBlock - 1 < out_width && bm * D + phase - H >= 0) {
#pragma unroll 4
        for (int k = 0; k < L; ++k) cext::cmac32(re, im, pk, k, xf[-(int64_t)k]);
    } else {
        const int64_t k_x = n < H ? n : H;  // taps 0..k_x meet x, the rest the history
        for (int64_t k = 0; k <= k_x; ++k) cext::cmac32(re, im, pk, k, xf[-k]);
        if (hist) {
            const uint32_t* __restrict__ hf = hist + r * H + H + n;  // frame n - k < 0 at hf[-k]
            for (int64_t k = k_x + 1; k <= H; ++k) cext::cmac32(re, im, pk, k, hf[-k]);
        }
    }
    cext::store_frame32<STAGE>(y, gi, re, im, shl, frac);
}

// hist_out[r, j] = X[r, width - H + j]: FrameT is uint32_t when all three arrays are 4-byte
// aligned (a frame is one dword), else a pair of int16.
struct cs_frame16 {
    int16_t re, im;
};
template <typename FrameT>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_stream_hist_kernel(const FrameT* __restrict__ x,
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

int64_t out_width(int64_t width, int decim, int phase) { return cext::decim_out_width(width, decim, phase); }

int next_phase(int64_t width, int decim, int phase) {
    if (width < 0 || decim < 1 || phase < 0 || phase >= decim) return -1;
    if (width <= phase) return (int)(phase - width);
    // width - phase = q * D + rem + 1 and out_width = q + 1: out_width * D - (width - phase) = D - 1 - rem
    return decim - 1 - (int)((width - phase - 1) % decim);
}

// cext::check_head (csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its
// order and its texts), then the header's checks 2 to 5.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase,
          int frac, int acc_bits, int stage, int64_t* ow, std::string* err) {
    if (const int rc = cext::check_head(rows, width, hq, L, frac, acc_bits, stage, err)) return rc;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    int64_t rw = 0, rh = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || rw > INT64_MAX / 8)
        return *err = "rows * width * 2 * 4 bytes must fit in int64", FIR_EINVAL;
    if (__builtin_mul_overflow(rows, (int64_t)(L - 1), &rh) || rh > INT64_MAX / 4)
        return *err = "rows * (taps - 1) * 4 bytes must fit in int64", FIR_EINVAL;
    *ow = out_width(width, decim, phase);
    if (rw != 0 && !x) return *err = "x and y must not be NULL", FIR_EINVAL;
    if (rows != 0 && *ow != 0 && !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    return FIR_OK;
}

int route_of(uintptr_t x, uintptr_t hist_in, uintptr_t y, uintptr_t hist_out, int64_t rows, int64_t width, int64_t ow,
             const int32_t* hq, int L, int decim, int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    // a frame of a history is one dword to the 32-bit kernels (NULL and taps = 1: no history is read)
    const bool h4 = L == 1 || (hist_in % 4 == 0 && hist_out % 4 == 0);
    if (d2 && h4 && cext::tile_route_ok(x, rows, width, ow, L, decim, stage, bucket)) return FIR_CSTREAM_FAST;
    if (d2 && h4 && x % 4 == 0) return FIR_CSTREAM_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CSTREAM_GENERIC128 : FIR_CSTREAM_GENERIC64;
}

// what the calling thread's last launch() launched as its FIR kernel: those go through
// cext::launch_recorded, the history kernel does not
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

static hipError_t launch_fast(int bucket, const void* x, const void* hist, void* y, int64_t rows, int64_t width,
                              int64_t ow, const int32_t* hq, int L, int D, int phase, int frac, int acc_bits,
                              hipStream_t s) {
    return cext::with_tile_bucket(bucket, [&](auto lp) {
        constexpr int LP = decltype(lp)::value;
        const TapsCs<LP> t{cext::pack_window_taps<LP>(hq, L)};
        const cext::TileGeom g = cext::tile_geom(D, LP, rows, ow);
        const int base = phase - (L - 1);  // causal: output m's window starts at frame m * D + base of its row's stream
        if (acc_bits == 32)
            return launch_recorded(FIR_CSTREAM_FAST, LP, fir1d_cplx_stream_kernel<LP, true>, g.grid, g.lds, s, x, hist, y,
                                   width, ow, g.groups, g.G, D, base, L - 1, g.PL, g.magic, t, 0, frac);
        return launch_recorded(FIR_CSTREAM_FAST, LP, fir1d_cplx_stream_kernel<LP, false>, g.grid, g.lds, s, x, hist, y,
                               width, ow, g.groups, g.G, D, base, L - 1, g.PL, g.magic, t, 32 - acc_bits, frac);
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
        hipLaunchKernelGGL(fir1d_cplx_stream_hist_kernel<uint32_t>, grid, dim3(kBlock), 0, s, (const uint32_t*)x,
                           (const uint32_t*)hist_in, (uint32_t*)hist_out, n_hist, width, H);
    else
        hipLaunchKernelGGL(fir1d_cplx_stream_hist_kernel<cs_frame16>, grid, dim3(kBlock), 0, s, (const cs_frame16*)x,
                           (const cs_frame16*)hist_in, (cs_frame16*)hist_out, n_hist, width, H);
    return hipGetLastError();
}

int launch(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq, int L, int decim,
           int phase, int frac, int acc_bits, int stage, void* y, int16_t* hist_out, hipStream_t stream,
           std::string* err) {
    int64_t ow = 0;
    const int rc = check(x, y, rows, width, hq, L, decim, phase, frac, acc_bits, stage, &ow, err);
    if (rc) return rc;
    cext::launch_none();
    if (rows == 0) return FIR_OK;
    if (L == 1) hist_in = nullptr, hist_out = nullptr;  // no history: both pointers are ignored
    if (ow != 0) {
        int bucket = 0;
        const int route = route_of((uintptr_t)x, (uintptr_t)hist_in, (uintptr_t)y, (uintptr_t)hist_out, rows, width, ow,
                                   hq, L, decim, frac, acc_bits, stage, &bucket);
        hipError_t e;
        if (route == FIR_CSTREAM_FAST)
            e = launch_fast(bucket, x, hist_in, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits, stream);
        else
            e = fir::with_stage(stage, [&](auto st) {
                return cext::launch_generic(
                    route, FIR_CSTREAM_GENERIC32, FIR_CSTREAM_GENERIC128, fir1d_cplx_stream_generic32_kernel<st>,
                    fir1d_cplx_stream_generic_kernel<st, false>, fir1d_cplx_stream_generic_kernel<st, true>, rows * ow, hq,
                    L, frac, acc_bits, stream, [&](auto kernel, dim3 grid, const void* table, int t0, int t1) {
                        return launch_recorded(route, 0, kernel, grid, 0, stream, x, hist_in, y, rows * ow, width, ow,
                                               (int64_t)decim, (int64_t)phase, table, L, t0, t1);
                    });
            });
        if (e != hipSuccess)
            return *err = std::string("fir1d cplx stream launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    }
    if (hist_out) {
        const hipError_t e = launch_hist(x, hist_in, hist_out, rows, width, L - 1, stream);
        if (e != hipSuccess)
            return *err = std::string("fir1d cplx stream history launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    }
    return FIR_OK;
}

}  // namespace cstream
