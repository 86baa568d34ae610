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
// scatter, the output-run writer, the generic kernels' steps) and nothing compiled from either.
//
//  * fir1d_cplx_resample_kernel — the hot path (FIR_CRESAMPLE_FAST, see route_of): the decimator's
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
//    thread's loads (at most kCrMaxIt = 5) issued before its first LDS write.  A lane's period is D
//    dwords from the next lane's, so the dwords are stored as D polyphase planes, frame a (counted
//    from the workgroup's first window's first frame) at plane a mod D, index a / D: window dword
//    k of period w is at plane k mod D, index w + k / D, so consecutive lanes read consecutive
//    dwords for every D.  Every window element is a whole dword: no v_alignbit, no leading zero tap.
//
//    Taps.  Per q the sub-filter in window order, zero-padded to the tap bucket NP in {1, 2, 3, 4,
//    6, 8, 10, 12, 16, 20, 24, 28, 32}, as two packed tables passed BY VALUE next to the window's
//    first dword k0_q and a table of the LDS offset (k mod D) * PL + k / D of every window dword k
//    (read with scalar loads of consecutive entries inside a run-time loop over q): no device table,
//    nothing allocated, so the call can be captured in a graph.  cr_slots(NP) bounds U * NP for
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
using fir::dot2_acc;
using fir::IntTag;
using fir::kBlock;
using fir::OutTraits;

constexpr int kCrInBytes = 4096;    // input bytes a workgroup keeps in flight, at least
constexpr int kCrMinT = 256;        // the smallest tile and workgroup: one pass, one period per lane
constexpr int kCrOutBytes = 16384;  // T = P halved while T * U * 8 exceeds this
constexpr int kCrMaxUD = 16;        // 2 <= U, D <= 16
constexpr int kCrMaxTaps = 128;
constexpr int kCrMaxNP = 32;        // the largest tap bucket: ceil(L / U) of the fast path
constexpr int kCrOffs = 64;         // window dwords a lane can address: the highest k0 + NP is 17 + 32

// periods per workgroup
__host__ __device__ constexpr int cr_periods(int D) {
    int P = kCrMinT;
    while (P * D * 4 < kCrInBytes) P *= 2;
    return P;
}
// 16-byte chunks a workgroup of n periods stages: lead + the last period's first frame + ext, the
// frames from there to the end of the furthest window (the highest k0 + NP)
__host__ __device__ constexpr int cr_chunks(int lead, int n, int D, int ext) {
    return (lead + (n - 1) * D + ext + kChunk - 1) / kChunk;
}
constexpr int kCrMaxExt = kCrMaxUD + 1 + kCrMaxNP;  // k0 <= D + 1
constexpr int cr_max_chunks() {
    int m = 0;
    for (int D = 2; D <= kCrMaxUD; ++D) {
        const int c = cr_chunks(kChunk - 1, cr_periods(D), D, kCrMaxExt);
        m = c > m ? c : m;
    }
    return m;
}
constexpr int kCrMaxIt = (cr_max_chunks() + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kCrMaxIt == 5, "staging steps");
static_assert(kChunk * kCrMaxIt * kBlock < (1 << 14), "the magic division's range");
static_assert(kCrMaxExt <= kCrOffs, "the offset table holds every window dword");

// the tap buckets, and the one below a bucket (0 below the first)
constexpr int kCrBuckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, kCrMaxNP};
constexpr int cr_prev_bucket(int NP) {
    int prev = 0;
    for (const int b : kCrBuckets) {
        if (b >= NP) break;
        prev = b;
    }
    return prev;
}
// Dwords per tap table of bucket NP: U * NP for the largest U that can land in it.  A longest
// sub-filter of more than prev taps has ceil(L / U) > prev, so L >= U * prev + 1 and, with L <= 128,
// U <= 127 / prev.
constexpr int cr_slots(int NP) {
    const int prev = cr_prev_bucket(NP);
    const int umax = prev < 1 || (kCrMaxTaps - 1) / prev > kCrMaxUD ? kCrMaxUD : (kCrMaxTaps - 1) / prev;
    return umax * NP;
}
static_assert(cr_slots(1) == 16 && cr_slots(16) == 160 && cr_slots(kCrMaxNP) == 128, "tap table sizes");

template <int NP>
struct TapsCr {
    uint32_t a[cr_slots(NP)];  // phase q, window dword w at q * NP + w: (hr, -hi) of the tap that meets it
    uint32_t b[cr_slots(NP)];  //                                        (hi, hr); zero where no tap does
    uint32_t k0[kCrMaxUD];     // phase q: its window's first dword, from the period's first window dword
    uint32_t off[kCrOffs];     // window dword k of a period lies (k mod D) * PL + k / D dwords from its plane row
};

template <int NP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_resample_kernel(const uint32_t* __restrict__ x,
                                                                     int32_t* __restrict__ y, int64_t width,
                                                                     int64_t out_width, uint32_t groups, int U, int D,
                                                                     int P, int T, int S, int ext, int PL,
                                                                     uint32_t magic, TapsCr<NP> taps, int shl, int frac) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cr_lds[];  // D planes of PL dwords, then the output stage
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t v0 = (int64_t)tb * P;  // first period of the workgroup
    const int64_t m0 = v0 * U;           // ... and its first output frame
    const int TU = T * U;                // output frames per tile
    const int64_t left = (out_width - m0 + TU - 1) / TU;
    const int gt = left < P / T ? (int)left : P / T;  // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = v0 * D + S;                    // its first window's first frame (may be < 0)
    const int64_t o = a0 & ~(int64_t)(kChunk - 1);    // the first frame staged: floor to 4 frames
    const int lead = (int)(a0 - o);                   // 0..3
    const int nchunks = cr_chunks(lead, gt * T, D, ext);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row (zero outside [0, width)) in D planes; LDS
    // dword 0 is the first window's first frame a0 (the up to 3 frames in front of it are never read)
    cext::u4 raw[kCrMaxIt];
    cext::stage_load(raw, xr, o, nchunks, width, [&](int64_t f) { return f >= 0 && f < width ? xr[f] : 0u; });
    cext::scatter_planes(cr_lds, raw, nchunks, lead, D, PL, magic);
    __syncthreads();

    uint32_t* const outw = cr_lds + ((D * PL + 3) & ~3);
    const int u = threadIdx.x;
    const uint32_t vstep = (uint32_t)U * 8u;  // bytes from a period's outputs to the next period's
    for (int g = 0; g < gt; ++g) {
        const int64_t mg = m0 + (int64_t)g * TU;                          // the tile's first output frame
        const int no = out_width - mg < TU ? (int)(out_width - mg) : TU;  // its output frames inside the row
        char* const yt = reinterpret_cast<char*>(y + (r * out_width + mg) * 2);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(yt) & 15u);  // the stage's first byte

        // ---- lane u: the U output frames of period u of every pass (kBlock periods), into the stage
        for (int vp = u; vp < T && vp * U < no; vp += kBlock) {
            const uint32_t wrow = (uint32_t)(g * T + vp);  // its plane row: dword wrow * D is its first window dword
            uint32_t b = sh + (uint32_t)vp * vstep;        // period vp, output 0
            for (int q = 0; q < U; ++q, b += 8u) {
                const uint32_t* __restrict__ ta = taps.a + q * NP;  // wave-uniform
                const uint32_t* __restrict__ tq = taps.b + q * NP;
                const uint32_t* __restrict__ oo = taps.off + taps.k0[q];
                uint32_t re = 0, im = 0;
                // at most 16 window dwords at a time, so that a chunk's taps and offsets fit the SGPRs
                constexpr int NC = (NP + 15) / 16, CW = (NP + NC - 1) / NC;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c) __builtin_amdgcn_sched_barrier(0);
                    uint32_t d[CW];
#pragma unroll
                    for (int w = c * CW; w < (c + 1) * CW && w < NP; ++w) d[w - c * CW] = cr_lds[wrow + oo[w]];
#pragma unroll
                    for (int w = c * CW; w < (c + 1) * CW && w < NP; ++w) {
                        re = dot2_acc(d[w - c * CW], ta[w], re);
                        im = dot2_acc(d[w - c * CW], tq[w], im);
                    }
                }
                outw[cext::phys(b) >> 2] = (uint32_t)fir::round_acc<ACC32>(re, shl, frac);
                outw[cext::phys(b + 4u) >> 2] = (uint32_t)fir::round_acc<ACC32>(im, shl, frac);
            }
        }
        __syncthreads();

        // ---- the tile's output run [sh, end) of the stage, as 16-byte vectors at 16-byte addresses
        cext::write_run(outw, yt, sh, sh + (uint32_t)no * 8u);
        __syncthreads();  // the next tile overwrites the stage
    }
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

namespace {

// The U windows of a period.  Phase q: p the first tap, c the frame (from the period's first) that
// tap meets, n the taps, k0 the first dword of its window counted from S, the first frame of the
// lowest window; need: the longest sub-filter; kmax: the highest k0.
struct Plan {
    int S = 0, need = 0, kmax = 0;
    int p[kCrMaxUD] = {}, c[kCrMaxUD] = {}, n[kCrMaxUD] = {}, k0[kCrMaxUD] = {};
};

Plan plan_of(int L, int U, int D, int phase) {
    Plan pl;
    int lo = 0;
    bool any = false;
    for (int q = 0; q < U; ++q) {
        const int a = phase + L / 2 + q * D;
        pl.p[q] = a % U;
        pl.c[q] = a / U;
        pl.n[q] = pl.p[q] < L ? (L - pl.p[q] + U - 1) / U : 0;  // 0: an empty phase, its outputs are 0
        if (!pl.n[q]) continue;
        const int s = pl.c[q] - pl.n[q] + 1;
        if (!any || s < lo) lo = s;
        any = true;
        if (pl.n[q] > pl.need) pl.need = pl.n[q];
    }
    pl.S = lo;
    for (int q = 0; q < U; ++q) {
        if (!pl.n[q]) continue;
        pl.k0[q] = pl.c[q] - pl.n[q] + 1 - pl.S;  // >= 0
        if (pl.k0[q] > pl.kmax) pl.kmax = pl.k0[q];
    }
    return pl;
}

int bucket_of(int need) {
    for (const int b : kCrBuckets)
        if (need <= b) return b;
    return kCrMaxNP;
}

// periods per tile: the workgroup's periods, halved while the tile's outputs exceed kCrOutBytes
int tile_of(int P, int U) {
    int T = P;
    while (T > kCrMinT && T * U * 8 > kCrOutBytes) T /= 2;
    return T;
}

}  // namespace

int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int L, int up,
             int decim, int phase, int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    if (d2 && up >= 2 && up <= kCrMaxUD && decim >= 2 && decim <= kCrMaxUD && L <= kCrMaxTaps &&
        (L + up - 1) / up <= kCrMaxNP && stage == FIR_OUT_I32 && x % 16 == 0 &&
        (rows == 1 || width % kChunk == 0)) {  // every row starts as x does
        const int64_t per = (int64_t)cr_periods(decim) * up;  // output frames per workgroup
        const int64_t groups = (ow + per - 1) / per;
        // the grid is rows * groups < 2^31 workgroups; the kernel holds a group index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / groups) {
            *bucket = bucket_of(plan_of(L, up, decim, phase).need);
            return FIR_CRESAMPLE_FAST;
        }
    }
    if (d2 && x % 4 == 0) return FIR_CRESAMPLE_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CRESAMPLE_GENERIC128 : FIR_CRESAMPLE_GENERIC64;
}

// what the calling thread's last launch() launched: every kernel goes through cext::launch_recorded
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

template <int NP>
static hipError_t launch_fast_np(const void* x, void* y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int U,
                                 int D, const Plan& pl, int frac, int acc_bits, hipStream_t s) {
    const int P = cr_periods(D);
    const int ext = pl.kmax + NP;                           // window dwords a period can read
    const int chunks = cr_chunks(kChunk - 1, P, D, ext);    // lead <= 3
    // never taken: cr_slots bounds U * NP, kCrMaxExt the windows
    if (U * NP > cr_slots(NP) || ext > kCrOffs || chunks > kCrMaxIt * kBlock) return hipErrorInvalidValue;
    const int PL = (chunks * kChunk + D - 1) / D;  // dwords per plane
    TapsCr<NP> t = {};
    for (int k = 0; k < kCrOffs; ++k) t.off[k] = (uint32_t)((k % D) * PL + k / D);
    for (int q = 0; q < U; ++q) {
        t.k0[q] = (uint32_t)pl.k0[q];
        for (int w = 0; w < pl.n[q]; ++w) {  // window dword w is frame S + k0 + w = c - (n - 1 - w): tap n - 1 - w
            const int k = pl.p[q] + U * (pl.n[q] - 1 - w);
            const int32_t hr = hq[2 * k], hi = hq[2 * k + 1];
            const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
            t.a[q * NP + w] = r16 | (ni16 << 16);
            t.b[q * NP + w] = i16 | (r16 << 16);
        }
    }
    const int T = tile_of(P, U);
    const int in_dwords = (D * PL + 3) & ~3;
    const uint32_t stage_bytes = (uint32_t)(T * U * 8) + 16u;
    const size_t lds = (size_t)in_dwords * sizeof(uint32_t) + cext::phys(stage_bytes) + 4;
    const uint32_t magic = (1u << cext::kMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (ow + (int64_t)P * U - 1) / ((int64_t)P * U);
    const dim3 grid((unsigned)(rows * groups));
    if (acc_bits == 32)
        return launch_recorded(FIR_CRESAMPLE_FAST, NP, fir1d_cplx_resample_kernel<NP, true>, grid, lds, s,
                               (const uint32_t*)x, (int32_t*)y, width, ow, (uint32_t)groups, U, D, P, T, pl.S, ext, PL,
                               magic, t, 0, frac);
    return launch_recorded(FIR_CRESAMPLE_FAST, NP, fir1d_cplx_resample_kernel<NP, false>, grid, lds, s, (const uint32_t*)x,
                           (int32_t*)y, width, ow, (uint32_t)groups, U, D, P, T, pl.S, ext, PL, magic, t, 32 - acc_bits,
                           frac);
}

static hipError_t launch_fast(int bucket, const void* x, void* y, int64_t rows, int64_t width, int64_t ow,
                              const int32_t* hq, int L, int U, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    const Plan pl = plan_of(L, U, D, phase);
    const auto go = [&](auto np) {
        return launch_fast_np<decltype(np)::value>(x, y, rows, width, ow, hq, U, D, pl, frac, acc_bits, s);
    };
    switch (bucket) {
        case 1: return go(IntTag<1>{});
        case 2: return go(IntTag<2>{});
        case 3: return go(IntTag<3>{});
        case 4: return go(IntTag<4>{});
        case 6: return go(IntTag<6>{});
        case 8: return go(IntTag<8>{});
        case 10: return go(IntTag<10>{});
        case 12: return go(IntTag<12>{});
        case 16: return go(IntTag<16>{});
        case 20: return go(IntTag<20>{});
        case 24: return go(IntTag<24>{});
        case 28: return go(IntTag<28>{});
        default: return go(IntTag<kCrMaxNP>{});
    }
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
