// fir1d_cplx_resample.hip — the rational U/D resampling complex-tap 1-D fixed-point FIR for complex
// int16: zero-stuff by U, filter with complex taps, keep every D-th output frame, in one polyphase
// pass over x itself.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); c0 = L / 2
//   mid_width = width * U;  out_width = mid_width > phase ? (mid_width - phase + D - 1) / D : 0
//   a_q = phase + c0 + q*D, p_q = a_q mod U, c_q = a_q div U; output frame m = v*U + q (0 <= q < U)
//   meets the taps p_q + U*t only, t = 0 .. n_q - 1 (n_q taps: p_q + U*t < L):
//   re[m] = stage(round(wrap_acc( sum_t hr[p_q+U*t] * xr[v*D+c_q-t] - hi[p_q+U*t] * xi[v*D+c_q-t] )))
//   im[m] = stage(round(wrap_acc( sum_t hr[p_q+U*t] * xi[v*D+c_q-t] + hi[p_q+U*t] * xr[v*D+c_q-t] )))
//
// p_q and c_q depend on q alone and the pattern repeats every U output frames = D input frames (one
// PERIOD v).  The arithmetic is csrc/fir1d_cplx.hip's (frames outside a row are zero, one exact sum
// per part, wrapped once, overflow-free round-half-up, int32 or saturated-u8 stage).  This file is
// libfir_cresample.so's own device side; it shares the header-only device helpers of csrc/
// (fir_common.h, fir_dispatch.h) and of csrc_cext/ (cext_device.h: input staging, the plane
// scatter, the output-run writer, the resampling tile kernel's body, the generic kernels' steps) and
// nothing compiled from either.
//
//  * fir1d_cplx_resample_kernel — the hot path (FIR_CRESAMPLE_FAST, see route_of), a wrapper over
//    cext::resample_tile, which libfir_crstream.so runs with a causal plan and a history: the decimator's
//    input side, the interpolator's output side and the complex MAC.  One interleaved frame is one
//    dword, and v_dot2_i32_i16 of it against A = (hr, -hi) is the real part of one tap's product,
//    against B = (hi, hr) the imaginary part: two v_dot2 per sub-filter tap and output frame on
//    32-bit wrap-around accumulators (exact mod 2^32, all the wrap to acc_bits <= 32 needs; ACC32
//    skips the wrap).
//
//    Work split.  A workgroup of 256 lanes owns P consecutive periods of ONE row (never two rows, so
//    frames outside the row are zeroed once, at staging): P = 256 doubled until P * D * 4 >= 4096
//    bytes of input are in flight per workgroup (512 at D = 2 or 3, else 256).  It works through
//    them as tiles of T periods, T = P halved while the tile's T * U * 8 output bytes exceed 16 KiB,
//    but not below 256.  A tile is computed in passes of 256 periods: lane u owns period u of every
//    pass and produces its U output frames.  Grid: rows x ceil(out_width / (P * U)).
//
//    Input.  The workgroup stages the frames behind all of its outputs, from the 16-byte boundary at
//    or below the first one (lead = 0..3 frames), as dwords: 16-byte global loads, all of a
//    thread's loads (at most kRsMaxIt = 5) issued before its first LDS write.  A lane's period is D
//    dwords from the next lane's, so the dwords are stored as D polyphase planes, frame a (counted
//    from the workgroup's first window's first frame) at plane a mod D, index a / D: window dword
//    k of period w is at plane k mod D, index w + k / D, so consecutive lanes read consecutive
//    dwords for every D.  Every window element is a whole dword: no v_alignbit, no leading zero tap.
//
//    Taps.  Per q the sub-filter in window order, zero-padded to the tap bucket NP in {1, 2, 3, 4,
//    6, 8, 10, 12, 16, 20, 24, 28, 32}, as two packed tables passed BY VALUE next to the window's
//    first dword k0_q and a table of the LDS offset (k mod D) * PL + k / D of every window dword k
//    (read with scalar loads of consecutive entries inside a run-time loop over q): no device table,
//    nothing allocated, so the call can be captured in a graph.  rs_slots(NP) bounds U * NP for
//    every (L, U) that lands in a bucket: at most 160 dwords per table.  The window is taken at most
//    16 dwords at a time, so that a chunk's taps and offsets (3 x 16 dwords) fit the SGPRs.
//
//    Output, as in the interpolator.  Every result goes to an LDS output stage at the byte it has in
//    the tile's output run (byte b at b + 4 * (b / 128): one pad dword per 32), which starts
//    (y address mod 16) bytes in, so LDS vectors and global vectors line up for ANY int32 y address;
//    the run is then written as whole 16-byte vectors, consecutive lanes consecutive vectors, the
//    partial vector at either end dword by dword, inside the tile's own bytes.  The row's last
//    period is masked at m < out_width: the run ends there.
//
//    LDS per workgroup: D planes of PL dwords (about P * D + 64 dwords, at most 16.3 KiB) plus
//    T * U * 8 + 16 bytes of stage with its padding (at most 33 KiB at U = 16): under 50 KiB.
//
//  * The generic kernels — every other legal call: one output frame per thread, the interpolator's
//    generic kernels at j = m * D + phase, walking the taps k = p_e, p_e + U, ... whose frame lies in
//    the row (the in-row test as loop bounds), taps from a cached device table.
//    fir1d_cplx_resample_generic32_kernel (int16-sized parts, acc_bits <= 32, frac <= 31, x 4-byte
//    aligned): 32-bit wrap-around sums, two v_dot2 per tap over a packed (A, B) table.
//    fir1d_cplx_resample_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
#include <string>

#include "cresample.h"
#include "cext_launch.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cresample {

using cext::kChunk;  // frames per staging step of one thread (16 bytes)
using cext::launch_recorded;
using fir::kBlock;
using fir::OutTraits;

// The fast kernel's constants and tap buckets.  The kernel body and its tables are cext_device.h's
// (resample_tile, shared with libfir_crstream.so); the numbers this library's route and header rest
// on are stated here and held against the shared ones.
constexpr int kCrInBytes = 4096;    // input bytes a workgroup keeps in flight, at least
constexpr int kCrMinT = 256;        // the smallest tile and workgroup: one pass, one period per lane
constexpr int kCrOutBytes = 16384;  // T = P halved while T * U * 8 exceeds this
constexpr int kCrMaxUD = 16;        // 2 <= U, D <= 16
constexpr int kCrMaxTaps = 128;
constexpr int kCrMaxNP = 32;        // the largest tap bucket: ceil(L / U) of the fast path
constexpr int kCrBuckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, kCrMaxNP};
static_assert(kCrInBytes == cext::kRsInBytes && kCrMinT == cext::kRsMinT && kCrOutBytes == cext::kRsOutBytes &&
                  kCrMaxUD == cext::kRsMaxUD && kCrMaxTaps == cext::kRsMaxTaps && kCrMaxNP == cext::kRsMaxNP,
              "the shared kernel's constants");
constexpr bool cr_buckets_are_shared() {
    constexpr int n = sizeof(kCrBuckets) / sizeof(kCrBuckets[0]);
    if (n != sizeof(cext::kRsBuckets) / sizeof(cext::kRsBuckets[0])) return false;
    for (int i = 0; i < n; ++i)
        if (kCrBuckets[i] != cext::kRsBuckets[i]) return false;
    return true;
}
static_assert(cr_buckets_are_shared(), "the shared kernel's tap buckets");

// cext::ResampleTaps under the name the kernel's signature, and so its symbol, has always carried
template <int NP>
struct TapsCr : cext::ResampleTaps<NP> {};

template <int NP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_resample_kernel(const uint32_t* __restrict__ x,
                                                                     int32_t* __restrict__ y, int64_t width,
                                                                     int64_t out_width, uint32_t groups, int U, int D,
                                                                     int P, int T, int S, int ext, int PL,
                                                                     uint32_t magic, TapsCr<NP> taps, int shl, int frac) {
    cext::resample_tile<NP, ACC32, false>(x, nullptr, y, width, out_width, groups, U, D, P, T, S, ext, 0, PL, magic, taps,
                                          shl, frac);
}

// One output frame per thread: frame gi = r * out_width + m is frame j = m * D + phase = i * U + e
// of the interpolated row and sums the taps p_e + U * t whose frame i + c_e - t lies in row r;
// taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_resample_generic_kernel(
    const int16_t* __restrict__ x, typename OutTraits<STAGE>::T* __restrict__ y, int64_t n_out, int64_t width,
    int64_t out_width, int64_t U, int64_t D, int64_t phase, const int32_t* __restrict__ taps, int L, int frac,
    int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t j = m * D + phase;  // < width * U
    const cext::PolyWalk w = cext::poly_walk(j, U, L, width);
    const int16_t* __restrict__ xr = x + 2 * r * width;
    cext::Acc<WIDE> re = 0, im = 0;
    for (int64_t t = w.t_lo; t <= w.t_hi; ++t) cext::cmac<WIDE>(re, im, taps, w.pe + U * t, xr, w.n - t);
    cext::store_frame<STAGE, WIDE>(y, gi, re, im, frac, acc_bits);
}

// The same walk on 32-bit wrap-around accumulators over the packed table; a frame is one aligned dword.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_resample_generic32_kernel(
    const uint32_t* __restrict__ x, typename OutTraits<STAGE>::T* __restrict__ y, int64_t n_out, int64_t width,
    int64_t out_width, int64_t U, int64_t D, int64_t phase, const uint32_t* __restrict__ pk, int L, int shl, int frac) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t m = gi % out_width, r = gi / out_width;
    const int64_t j = m * D + phase;
    const cext::PolyWalk w = cext::poly_walk(j, U, L, width);
    const uint32_t* __restrict__ xf = x + r * width + w.n;  // tap pe + U * t meets frame xf[-t]
    uint32_t re = 0, im = 0;
    for (int64_t t = w.t_lo; t <= w.t_hi; ++t) cext::cmac32(re, im, pk, w.pe + U * t, xf[-t]);
    cext::store_frame32<STAGE>(y, gi, re, im, shl, frac);
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t out_width(int64_t width, int up, int decim, int phase) {
    int64_t mid = 0;
    if (width < 0 || up < 1 || decim < 1 || phase < 0 || phase >= decim || __builtin_mul_overflow(width, (int64_t)up, &mid))
        return -1;
    return mid > phase ? (mid - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

// csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its order and its texts
// (tests/test_cabi_cresample.py holds them against libfir_hip.so's), then the header's checks 2 to 4.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int decim,
          int phase, int frac, int acc_bits, int stage, int64_t* ow, std::string* err) {
    if (const int rc = cext::check_head(rows, width, hq, L, frac, acc_bits, stage, err)) return rc;
    if (up < 1) return *err = "up must be >= 1", FIR_EINVAL;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    *ow = out_width(width, up, decim, phase);
    int64_t ro = 0, rw = 0;
    if (*ow < 0 || __builtin_mul_overflow(rows, *ow, &ro) || ro > INT64_MAX / 8 || __builtin_mul_overflow(rows, width, &rw) ||
        rw > INT64_MAX / 4)
        return *err = "width * up, rows * out_width * 2 * 4 bytes and rows * width * 4 bytes must fit in int64", FIR_EINVAL;
    if (rows != 0 && *ow != 0 && (!x || !y)) return *err = "x and y must not be NULL", FIR_EINVAL;
    return FIR_OK;
}

int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int L, int up,
             int decim, int phase, int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    if (d2 && up >= 2 && up <= kCrMaxUD && decim >= 2 && decim <= kCrMaxUD && L <= kCrMaxTaps &&
        (L + up - 1) / up <= kCrMaxNP && stage == FIR_OUT_I32 && x % 16 == 0 &&
        (rows == 1 || width % kChunk == 0)) {  // every row starts as x does
        const int64_t per = (int64_t)cext::rs_periods(decim) * up;  // output frames per workgroup
        const int64_t groups = (ow + per - 1) / per;
        // the grid is rows * groups < 2^31 workgroups; the kernel holds a group index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / groups) {
            *bucket = cext::rs_bucket_of(cext::rs_plan_of(L, up, decim, phase, L / 2).need);
            return FIR_CRESAMPLE_FAST;
        }
    }
    if (d2 && x % 4 == 0) return FIR_CRESAMPLE_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CRESAMPLE_GENERIC128 : FIR_CRESAMPLE_GENERIC64;
}

// what the calling thread's last launch() launched: every kernel goes through cext::launch_recorded
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

static hipError_t launch_fast(int bucket, const void* x, void* y, int64_t rows, int64_t width, int64_t ow,
                              const int32_t* hq, int L, int U, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    const cext::RsPlan pl = cext::rs_plan_of(L, U, D, phase, L / 2);  // centred: the one-shot entry's shift
    return cext::with_rs_bucket(bucket, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        cext::RsGeom g;
        TapsCr<NP> t = {};
        if (!cext::rs_setup<NP>(hq, U, D, pl, rows, ow, &g, &t)) return hipErrorInvalidValue;  // never taken
        if (acc_bits == 32)
            return launch_recorded(FIR_CRESAMPLE_FAST, NP, fir1d_cplx_resample_kernel<NP, true>, g.grid, g.lds, s,
                                   (const uint32_t*)x, (int32_t*)y, width, ow, g.groups, U, D, g.P, g.T, pl.S, g.ext, g.PL,
                                   g.magic, t, 0, frac);
        return launch_recorded(FIR_CRESAMPLE_FAST, NP, fir1d_cplx_resample_kernel<NP, false>, g.grid, g.lds, s,
                               (const uint32_t*)x, (int32_t*)y, width, ow, g.groups, U, D, g.P, g.T, pl.S, g.ext, g.PL,
                               g.magic, t, 32 - acc_bits, frac);
    });
}

int launch(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int decim, int phase,
           int frac, int acc_bits, int stage, void* y, hipStream_t stream, std::string* err) {
    int64_t ow = 0;
    const int rc = check(x, y, rows, width, hq, L, up, decim, phase, frac, acc_bits, stage, &ow, err);
    if (rc) return rc;
    cext::launch_none();
    if (rows == 0 || ow == 0) return FIR_OK;
    int bucket = 0;
    const int route = route_of((uintptr_t)x, (uintptr_t)y, rows, width, ow, hq, L, up, decim, phase, frac, acc_bits,
                               stage, &bucket);
    hipError_t e;
    if (route == FIR_CRESAMPLE_FAST)
        e = launch_fast(bucket, x, y, rows, width, ow, hq, L, up, decim, phase, frac, acc_bits, stream);
    else
        e = fir::with_stage(stage, [&](auto st) {
            return cext::launch_generic(
                route, FIR_CRESAMPLE_GENERIC32, FIR_CRESAMPLE_GENERIC128, fir1d_cplx_resample_generic32_kernel<st>,
                fir1d_cplx_resample_generic_kernel<st, false>, fir1d_cplx_resample_generic_kernel<st, true>, rows * ow, hq,
                L, frac, acc_bits, stream, [&](auto kernel, dim3 grid, const void* table, int t0, int t1) {
                    return launch_recorded(route, 0, kernel, grid, 0, stream, x, y, rows * ow, width, ow, (int64_t)up,
                                           (int64_t)decim, (int64_t)phase, table, L, t0, t1);
                });
        });
    if (e != hipSuccess) return *err = std::string("fir1d cplx resample launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace cresample
