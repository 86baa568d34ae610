// fir1d_cplx_decim.hip — the decimating complex-tap 1-D fixed-point FIR for complex int16: filter
// with complex taps and keep every D-th output frame, in one pass that computes only the kept frames.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); c = L / 2
//   out_width = width > phase ? (width - phase + D - 1) / D : 0;   n = m * D + phase
//   re[m] = stage(round(wrap_acc( sum_k hr[k] * xr[n-k+c] - hi[k] * xi[n-k+c] )))
//   im[m] = stage(round(wrap_acc( sum_k hr[k] * xi[n-k+c] + hi[k] * xr[n-k+c] )))
//
// The arithmetic is csrc/fir1d_cplx.hip's (frames outside a row are zero, one exact sum per part,
// wrapped once, overflow-free round-half-up, int32 or saturated-u8 stage), the tiling
// csrc/fir1d_decim.hip's.  This file is libfir_cdecim.so's own device side; it shares the
// header-only device helpers of csrc/ (fir_common.h, fir_dispatch.h) and of csrc_cext/
// (cext_device.h) and nothing compiled from either.
//
//  * fir1d_cplx_decim_kernel — the hot path (FIR_CDECIM_FAST, see route_of): cext_device.h's
//    decimating tile kernel (its comment describes the tiling, the D LDS planes, the magic division
//    and the stepped MAC loop) with a centred window origin, base = phase + L / 2 - (L - 1), and
//    frames outside the row staged as zero.  46 VGPRs at LP = 64, so the LDS (four workgroups per
//    CU), not the registers, sets the occupancy.  Measured at 64 taps, 2^26 frames, D = 2 / 8 / 16
//    (profiles/cdecim): 441 / 191 / 139 us with the MAC loop unrolled whole (hipcc hoists all 128
//    reads: 202 VGPRs, two workgroups per CU), 379 / 111 / 70 us in steps with each read next to its
//    MACs (one read in flight per wave), 241 / 79 / 56 us as committed.
//
//  * The generic kernels — every other legal call: one kept output frame per thread, walking the
//    taps whose frame lies in the row (the in-row test as loop bounds), taps from a cached device
//    table.  fir1d_cplx_decim_generic32_kernel (int16-sized parts, acc_bits <= 32, frac <= 31, x
//    4-byte aligned): 32-bit wrap-around sums, two v_dot2 per tap over a packed (A, B) table, and a
//    wave-uniform untested loop for workgroups whose windows all lie inside one row.
//    fir1d_cplx_decim_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
#include <string>

#include "cdecim.h"
#include "cext_launch.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cdecim {

using cext::launch_recorded;
using fir::kBlock;
using fir::OutTraits;

// cext::TileTaps under the name the kernel's signature, and so its symbol, has always carried
template <int LP>
struct TapsCd : cext::TileTaps<LP> {};

template <int LP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_decim_kernel(const uint32_t* __restrict__ x,
                                                                  int32_t* __restrict__ y, int64_t width,
                                                                  int64_t out_width, uint32_t groups, int G, int D,
                                                                  int base, int PL, uint32_t magic, TapsCd<LP> taps,
                                                                  int shl, int frac) {
    cext::decim_tile<LP, ACC32, false>(x, nullptr, y, width, out_width, groups, G, D, base, 0, PL, magic, taps, shl,
                                       frac);
}

// One kept output frame per thread: frame gi = r * out_width + m sums the taps k whose frame
// m * D + phase + c - k lies in row r; taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_decim_generic_kernel(const int16_t* __restrict__ x,
                                                                          typename OutTraits<STAGE>::T* __restrict__ y,
                                                                          int64_t n_out, int64_t width,
                                                                          int64_t out_width, int64_t D, int64_t phase,
                                                                          const int32_t* __restrict__ taps, int L,
                                                                          int frac, int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t n = m * D + phase + L / 2;  // tap k reads frame n - k
    // 0 <= n - k < width  <=>  n - width < k <= n
    const int64_t k_lo = n - width + 1 > 0 ? n - width + 1 : 0;
    const int64_t k_hi = n < L - 1 ? n : L - 1;
    const int16_t* __restrict__ xr = x + 2 * r * width;
    cext::Acc<WIDE> re = 0, im = 0;
    for (int64_t k = k_lo; k <= k_hi; ++k) cext::cmac<WIDE>(re, im, taps, k, xr, n - k);
    cext::store_frame<STAGE, WIDE>(y, gi, re, im, frac, acc_bits);
}

// The same walk on 32-bit wrap-around accumulators over the packed table; a frame is one aligned dword.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_decim_generic32_kernel(
    const uint32_t* __restrict__ x, typename OutTraits<STAGE>::T* __restrict__ y, int64_t n_out, int64_t width,
    int64_t out_width, int64_t D, int64_t phase, const uint32_t* __restrict__ pk, int L, int shl, int frac) {
    const int64_t b0 = (int64_t)blockIdx.x * kBlock;
    const int64_t gi = b0 + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t n = m * D + phase + L / 2;
    const uint32_t* __restrict__ xf = x + r * width + n;  // tap k meets frame xf[-k]
    uint32_t re = 0, im = 0;
    // A workgroup whose 256 outputs lie in one row, with every window inside it (known from its
    // first output, so the same for every lane), walks all L taps without a test: the loop is
    // wave-uniform and its taps come by scalar loads.  At a row's ends each lane walks the taps
    // its row meets.
    const int64_t bm = b0 % out_width;
    if (bm + kBlock - 1 < out_width && bm * D + phase + L / 2 - (L - 1) >= 0 &&
        (bm + kBlock - 1) * D + phase + L / 2 < width) {
#pragma unroll 4
        for (int k = 0; k < L; ++k) cext::cmac32(re, im, pk, k, xf[-(int64_t)k]);
    } else {
        const int64_t k_lo = n - width + 1 > 0 ? n - width + 1 : 0;
        const int64_t k_hi = n < L - 1 ? n : L - 1;
        for (int64_t k = k_lo; k <= k_hi; ++k) cext::cmac32(re, im, pk, k, xf[-k]);
    }
    cext::store_frame32<STAGE>(y, gi, re, im, shl, frac);
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t out_width(int64_t width, int decim, int phase) { return cext::decim_out_width(width, decim, phase); }

// csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its order and its texts
// (tests/test_cabi_cdecim.py holds them against libfir_hip.so's), then the header's checks 2 to 5.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase,
          int frac, int acc_bits, int stage, int64_t* ow, std::string* err) {
    if (const int rc = cext::check_head(rows, width, hq, L, frac, acc_bits, stage, err)) return rc;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    int64_t rw = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || rw > INT64_MAX / 8)
        return *err = "rows * width * 2 * 4 bytes must fit in int64", FIR_EINVAL;
    *ow = out_width(width, decim, phase);
    if (rows != 0 && *ow != 0 && (!x || !y)) return *err = "x and y must not be NULL", FIR_EINVAL;
    return FIR_OK;
}

int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int L, int decim,
             int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    if (d2 && cext::tile_route_ok(x, rows, width, ow, L, decim, stage, bucket)) return FIR_CDECIM_FAST;
    if (d2 && x % 4 == 0) return FIR_CDECIM_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CDECIM_GENERIC128 : FIR_CDECIM_GENERIC64;
}

// what the calling thread's last launch() launched: every kernel goes through cext::launch_recorded
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

static hipError_t launch_fast(int bucket, const void* x, void* y, int64_t rows, int64_t width, int64_t ow,
                              const int32_t* hq, int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    return cext::with_tile_bucket(bucket, [&](auto lp) {
        constexpr int LP = decltype(lp)::value;
        const TapsCd<LP> t{cext::pack_window_taps<LP>(hq, L)};
        const cext::TileGeom g = cext::tile_geom(D, LP, rows, ow);
        const int base = phase + L / 2 - (L - 1);  // output m's window starts at frame m * D + base of its row
        if (acc_bits == 32)
            return launch_recorded(FIR_CDECIM_FAST, LP, fir1d_cplx_decim_kernel<LP, true>, g.grid, g.lds, s, x, y, width,
                                   ow, g.groups, g.G, D, base, g.PL, g.magic, t, 0, frac);
        return launch_recorded(FIR_CDECIM_FAST, LP, fir1d_cplx_decim_kernel<LP, false>, g.grid, g.lds, s, x, y, width, ow,
                               g.groups, g.G, D, base, g.PL, g.magic, t, 32 - acc_bits, frac);
    });
}

int launch(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase, int frac,
           int acc_bits, int stage, void* y, hipStream_t stream, std::string* err) {
    int64_t ow = 0;
    const int rc = check(x, y, rows, width, hq, L, decim, phase, frac, acc_bits, stage, &ow, err);
    if (rc) return rc;
    cext::launch_none();
    if (rows == 0 || ow == 0) return FIR_OK;
    int bucket = 0;
    const int route = route_of((uintptr_t)x, (uintptr_t)y, rows, width, ow, hq, L, decim, frac, acc_bits, stage, &bucket);
    hipError_t e;
    if (route == FIR_CDECIM_FAST)
        e = launch_fast(bucket, x, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits, stream);
    else
        e = fir::with_stage(stage, [&](auto st) {
            return cext::launch_generic(
                route, FIR_CDECIM_GENERIC32, FIR_CDECIM_GENERIC128, fir1d_cplx_decim_generic32_kernel<st>,
                fir1d_cplx_decim_generic_kernel<st, false>, fir1d_cplx_decim_generic_kernel<st, true>, rows * ow, hq, L, frac,
                acc_bits, stream, [&](auto kernel, dim3 grid, const void* table, int t0, int t1) {
                    return launch_recorded(route, 0, kernel, grid, 0, stream, x, y, rows * ow, width, ow, (int64_t)decim,
                                           (int64_t)phase, table, L, t0, t1);
                });
        });
    if (e != hipSuccess) return *err = std::string("fir1d cplx decim launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace cdecim
