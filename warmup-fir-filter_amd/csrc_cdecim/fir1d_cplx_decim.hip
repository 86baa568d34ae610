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
// csrc/fir1d_decim.hip's.  This file is the whole device side of libfir_cdecim.so; it shares the
// header-only device helpers of csrc/ (fir_common.h, fir_dispatch.h) and nothing compiled from it.
//
//  * fir1d_cplx_decim_kernel — the hot path (FIR_CDECIM_FAST, see route_of).  One interleaved frame
//    is one dword, and v_dot2_i32_i16 of it against A = (hr, -hi) is the real part of one tap's
//    product, against B = (hi, hr) the imaginary part: two v_dot2 per tap and KEPT frame on 32-bit
//    wrap-around accumulators (exact mod 2^32, all the wrap to acc_bits <= 32 needs; ACC32 skips
//    the wrap).  Every window element is a whole dword, so no D needs a v_alignbit.  The taps are
//    reversed into window order and zero-padded at the window's far end to a bucket length LP in
//    {2, 4, 6, 8, 12, 16, 24, 32, 48, 64}; both tables travel BY VALUE in the kernel arguments
//    (scalar loads; no device table, nothing allocated: the call can be captured in a graph).
//
//    Tiling.  A tile is kCdT = 512 consecutive output frames of ONE row (never two rows, so frames
//    outside the row are zeroed once, at staging).  A workgroup of 256 lanes owns G = max(1, 16 / D)
//    consecutive tiles of its row and stages the (G * 512 - 1) * D + LP input frames behind them,
//    from the 16-byte boundary at or below the first one (lead = 0..3 frames), as dwords in LDS:
//    16-byte global loads, all of a thread's loads (at most kCdMaxIt = 9) issued before its first
//    LDS write.  At most 8257 frames = 32.3 KiB of LDS: four workgroups per CU.  Grid: rows x groups.
//
//    LDS layout.  Kept outputs are D dwords apart, so a linear window would put the lanes of a
//    ds_read_b32 D dwords apart (a 16-way bank conflict at D = 16).  Staged frame a is stored at
//    plane a mod D, index a / D (the magic multiply of fir1d_decim.hip, a < 2^14): window dword p
//    of output j of tile g is then at plane (lead + p) mod D, index (lead + p) / D + 512 g + j --
//    plane and index base are wave-uniform, and consecutive lanes read consecutive dwords: conflict
//    free for every D.  Lane u owns outputs u and u + 256 of each tile (one ds_read_b32 each per
//    window dword) and stores each as 8 bytes at int32 alignment, 512 contiguous bytes per wave,
//    non-temporal (y is written once and not read here).
//
//    The MAC loop takes the window in steps of cd_step(LP) <= 16 dwords: the step's 2 x 16 LDS
//    reads are issued together, then its 4 x 16 v_dot2 run; the steps are a real loop with the taps
//    indexed in the kernel arguments (still scalar loads).  46 VGPRs at LP = 64, so the LDS (four
//    workgroups per CU), not the registers, sets the occupancy.  Measured at 64 taps, 2^26 frames,
//    D = 2 / 8 / 16 (profiles/cdecim): 441 / 191 / 139 us with the loop unrolled whole (hipcc hoists
//    all 128 reads: 202 VGPRs, two workgroups per CU), 379 / 111 / 70 us in steps with each read
//    next to its MACs (one read in flight per wave), 241 / 79 / 56 us as committed.
//
//  * The generic kernels — every other legal call: one kept output frame per thread, walking the
//    taps whose frame lies in the row (the in-row test as loop bounds), taps from a cached device
//    table.  fir1d_cplx_decim_generic32_kernel (int16-sized parts, acc_bits <= 32, frac <= 31, x
//    4-byte aligned): 32-bit wrap-around sums, two v_dot2 per tap over a packed (A, B) table, and a
//    wave-uniform untested loop for workgroups whose windows all lie inside one row.
//    fir1d_cplx_decim_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "cdecim.h"
#include "cext_launch.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cdecim {

using cext::dot2_ok;
using cext::launch_recorded;
using cext::needs_wide;
using cext::table_locked;
using fir::dot2_acc;
using fir::IntTag;
using fir::kBlock;
using fir::OutTraits;

constexpr int kCdT = 512;         // output frames per tile: 2 per lane
constexpr int kCdMaxD = 16;       // G * D <= kCdMaxD: tiles per workgroup G = max(1, 16 / D)
constexpr int kCdMaxTaps = 64;    // the largest tap bucket
constexpr int kCdChunk = 4;       // frames per staging step of one thread (16 bytes)
// a / D == (a * (2^18 / D + 1)) >> 18 for a < 2^14 and 2 <= D <= 16, the product staying below 2^31 + 2^14
constexpr int kCdMagicShift = 18;

// 16-byte chunks a workgroup of G tiles stages: lead + the last window's start + LP frames
__host__ __device__ constexpr int cd_chunks(int lead, int G, int D, int LP) {
    return (lead + (G * kCdT - 1) * D + LP + kCdChunk - 1) / kCdChunk;
}
constexpr int cd_tiles_per_group(int D) { return D >= kCdMaxD ? 1 : kCdMaxD / D; }
constexpr int cd_max_chunks() {
    int m = 0;
    for (int D = 2; D <= kCdMaxD; ++D) {
        const int c = cd_chunks(kCdChunk - 1, cd_tiles_per_group(D), D, kCdMaxTaps);
        m = c > m ? c : m;
    }
    return m;
}
constexpr int kCdMaxIt = (cd_max_chunks() + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kCdMaxIt == 9, "staging steps");
static_assert(kCdChunk * cd_max_chunks() < (1 << 14), "the magic division's range");

// window dwords per step of the MAC loop: the whole window up to 16 taps, 12 or 16 of it beyond
constexpr int cd_step(int LP) { return LP <= 16 ? LP : (LP % 16 == 0 ? 16 : 12); }

typedef uint32_t cd_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t cd_u2_a4 __attribute__((ext_vector_type(2), aligned(4)));  // a store at int32 alignment

template <int LP>
struct TapsCd {
    uint32_t a[LP];  // window frame p meets tap k = L - 1 - p (zero for p >= L): a[p] = (hr, -hi)
    uint32_t b[LP];  //                                                          b[p] = (hi, hr)
};

template <int LP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_decim_kernel(const uint32_t* __restrict__ x,
                                                                  int32_t* __restrict__ y, int64_t width,
                                                                  int64_t out_width, uint32_t groups, int G, int D,
                                                                  int base, int PL, uint32_t magic, TapsCd<LP> taps,
                                                                  int shl, int frac) {
    constexpr int PB = cd_step(LP);
    static_assert(LP % PB == 0, "whole steps");
    extern __shared__ __attribute__((aligned(16))) uint32_t cd_lds[];  // D planes of PL dwords
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t m0 = (int64_t)tb * G * kCdT;     // first output frame of the workgroup
    const int64_t left = (out_width - m0 + kCdT - 1) / kCdT;
    const int gt = left < G ? (int)left : G;       // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = m0 * D + base;              // its first window's first frame in the row (may be < 0)
    const int64_t o = a0 & ~(int64_t)(kCdChunk - 1);  // LDS origin: floor to 4 frames
    const int lead = (int)(a0 - o);                // 0..3
    const int nchunks = cd_chunks(lead, gt, D, LP);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row (zero outside [0, width)): first every load
    // of the thread, then the LDS writes
    uint32_t raw[kCdMaxIt][kCdChunk];
#pragma unroll
    for (int it = 0; it < kCdMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kCdChunk;
        if (f >= 0 && f + kCdChunk <= width) {
            const cd_u4 q = *reinterpret_cast<const cd_u4*>(xr + f);
            raw[it][0] = q.x;
            raw[it][1] = q.y;
            raw[it][2] = q.z;
            raw[it][3] = q.w;
        } else {  // a chunk that crosses a row end, or lies outside the row
#pragma unroll
            for (int j = 0; j < kCdChunk; ++j) raw[it][j] = f + j >= 0 && f + j < width ? xr[f + j] : 0u;
        }
    }
#pragma unroll
    for (int it = 0; it < kCdMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
#pragma unroll
        for (int i = 0; i < kCdChunk; ++i) {
            const uint32_t a = (uint32_t)kCdChunk * (uint32_t)k + i;
            // every factor is below 2^24: v_mul_u32_u24 (full rate) instead of v_mul_lo_u32
            const uint32_t idx = (uint32_t)__umul24(a, magic) >> kCdMagicShift;  // a / D
            const uint32_t pl = a - (uint32_t)__umul24(idx, (uint32_t)D);        // a % D
            cd_lds[(uint32_t)__umul24(pl, (uint32_t)PL) + idx] = raw[it][i];
        }
    }
    __syncthreads();

    // ---- lane u: outputs u and u + 256 of each tile g; tile g's windows are 512 g plane rows on
    const int u = threadIdx.x;
    const uint32_t idx0 = ((uint32_t)lead * magic) >> kCdMagicShift;
    const uint32_t pl0 = (uint32_t)lead - idx0 * (uint32_t)D;
    const uint32_t wrap = (uint32_t)D * PL - 1;
    for (int g = 0; g < gt; ++g) {
        uint32_t re0 = 0, im0 = 0, re1 = 0, im1 = 0;
        uint32_t pl = pl0, off = pl0 * PL + idx0 + g * kCdT;  // wave-uniform: the plane and pl * PL + index
        // cd_step(LP) window dwords at a time: first the step's reads, then its MACs (header comment)
#pragma unroll 1
        for (int pb = 0; pb < LP; pb += PB) {
            uint32_t d0[PB], d1[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                d0[q] = cd_lds[off + u];
                d1[q] = cd_lds[off + u + kCdT / 2];
                off += PL;
                if (++pl == (uint32_t)D) {  // the next plane row: back (D - 1) planes, one index on
                    pl = 0;
                    off -= wrap;
                }
            }
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                re0 = dot2_acc(d0[q], taps.a[pb + q], re0);
                im0 = dot2_acc(d0[q], taps.b[pb + q], im0);
                re1 = dot2_acc(d1[q], taps.a[pb + q], re1);
                im1 = dot2_acc(d1[q], taps.b[pb + q], im1);
            }
        }
        const int64_t m = m0 + (int64_t)g * kCdT + u;
        int32_t* yo = y + (r * out_width + m) * 2;
        if (m < out_width)  // false only in the row's last tile
            __builtin_nontemporal_store(cd_u2_a4{(uint32_t)fir::round_acc<ACC32>(re0, shl, frac),
                                                 (uint32_t)fir::round_acc<ACC32>(im0, shl, frac)},
                                        reinterpret_cast<cd_u2_a4*>(yo));
        if (m + kCdT / 2 < out_width)
            __builtin_nontemporal_store(cd_u2_a4{(uint32_t)fir::round_acc<ACC32>(re1, shl, frac),
                                                 (uint32_t)fir::round_acc<ACC32>(im1, shl, frac)},
                                        reinterpret_cast<cd_u2_a4*>(yo + 2 * (kCdT / 2)));
    }
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
    using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
    using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;
    Acc re = 0, im = 0;
    for (int64_t k = k_lo; k <= k_hi; ++k) {
        const int64_t hr = taps[2 * k], hi = taps[2 * k + 1];
        const int64_t f = n - k;
        const int64_t ar = xr[2 * f], ai = xr[2 * f + 1];
        re += (Acc)(SAcc)(hr * ar) - (Acc)(SAcc)(hi * ai);
        im += (Acc)(SAcc)(hr * ai) + (Acc)(SAcc)(hi * ar);
    }
    if constexpr (WIDE) {
        y[2 * gi] = fir::stage_out128<STAGE>(fir::round128((__int128)re, frac, acc_bits));
        y[2 * gi + 1] = fir::stage_out128<STAGE>(fir::round128((__int128)im, frac, acc_bits));
    } else {
        y[2 * gi] = fir::stage_out<STAGE>(fir::round64((int64_t)re, frac, acc_bits));
        y[2 * gi + 1] = fir::stage_out<STAGE>(fir::round64((int64_t)im, frac, acc_bits));
    }
}

// The same walk on 32-bit wrap-around accumulators: pk[2k] = (hr[k], -hi[k]), pk[2k + 1] =
// (hi[k], hr[k]), two v_dot2_i32_i16 per tap; a frame is one aligned dword.
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
        for (int k = 0; k < L; ++k) {
            const uint32_t d = xf[-(int64_t)k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
    } else {
        const int64_t k_lo = n - width + 1 > 0 ? n - width + 1 : 0;
        const int64_t k_hi = n < L - 1 ? n : L - 1;
        for (int64_t k = k_lo; k <= k_hi; ++k) {
            const uint32_t d = xf[-k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
    }
    y[2 * gi] = fir::stage_out32<STAGE>(fir::round32(re, shl, frac));
    y[2 * gi + 1] = fir::stage_out32<STAGE>(fir::round32(im, shl, frac));
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t out_width(int64_t width, int decim, int phase) {
    if (width < 0 || decim < 1 || phase < 0 || phase >= decim) return -1;
    return width > phase ? (width - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

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

static int bucket_of(int L) {
    for (const int b : {2, 4, 6, 8, 12, 16, 24, 32, 48})
        if (L <= b) return b;
    return kCdMaxTaps;
}

int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int L, int decim,
             int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = dot2_ok(hq, L, frac, acc_bits);
    if (d2 && decim >= 2 && decim <= kCdMaxD && L <= kCdMaxTaps && stage == FIR_OUT_I32 && x % 16 == 0 &&
        (rows == 1 || width % kCdChunk == 0)) {  // every row starts as x does
        const int64_t tiles = (ow + kCdT - 1) / kCdT;
        // the grid is at most rows * tiles < 2^31 workgroups; the kernel holds a tile index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / tiles) {
            *bucket = bucket_of(L);
            return FIR_CDECIM_FAST;
        }
    }
    if (d2 && x % 4 == 0) return FIR_CDECIM_GENERIC32;
    return needs_wide(hq, L, acc_bits) ? FIR_CDECIM_GENERIC128 : FIR_CDECIM_GENERIC64;
}

// what the calling thread's last launch() launched: every kernel goes through cext::launch_recorded
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

template <int LP>
static hipError_t launch_fast_lp(const void* x, void* y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq,
                                 int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    TapsCd<LP> t;
    for (int p = 0; p < LP; ++p) {
        const int32_t hr = p < L ? hq[2 * (L - 1 - p)] : 0, hi = p < L ? hq[2 * (L - 1 - p) + 1] : 0;
        const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
        t.a[p] = r16 | (ni16 << 16);
        t.b[p] = i16 | (r16 << 16);
    }
    const int base = phase + L / 2 - (L - 1);  // output m's window starts at frame m * D + base of its row
    const int G = cd_tiles_per_group(D);
    const int PL = (cd_chunks(kCdChunk - 1, G, D, LP) * kCdChunk + D - 1) / D;  // dwords per plane
    const uint32_t magic = (1u << kCdMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (ow + (int64_t)G * kCdT - 1) / ((int64_t)G * kCdT);
    const size_t lds = (size_t)D * PL * sizeof(uint32_t);
    const dim3 grid((unsigned)(rows * groups));
    if (acc_bits == 32)
        return launch_recorded(FIR_CDECIM_FAST, LP, fir1d_cplx_decim_kernel<LP, true>, grid, lds, s, (const uint32_t*)x,
                               (int32_t*)y, width, ow, (uint32_t)groups, G, D, base, PL, magic, t, 0, frac);
    return launch_recorded(FIR_CDECIM_FAST, LP, fir1d_cplx_decim_kernel<LP, false>, grid, lds, s, (const uint32_t*)x,
                           (int32_t*)y, width, ow, (uint32_t)groups, G, D, base, PL, magic, t, 32 - acc_bits, frac);
}

static hipError_t launch_fast(int bucket, const void* x, void* y, int64_t rows, int64_t width, int64_t ow,
                              const int32_t* hq, int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    const auto go = [&](auto lp) {
        return launch_fast_lp<decltype(lp)::value>(x, y, rows, width, ow, hq, L, D, phase, frac, acc_bits, s);
    };
    switch (bucket) {
        case 2: return go(IntTag<2>{});
        case 4: return go(IntTag<4>{});
        case 6: return go(IntTag<6>{});
        case 8: return go(IntTag<8>{});
        case 12: return go(IntTag<12>{});
        case 16: return go(IntTag<16>{});
        case 24: return go(IntTag<24>{});
        case 32: return go(IntTag<32>{});
        case 48: return go(IntTag<48>{});
        default: return go(IntTag<kCdMaxTaps>{});
    }
}

template <int STAGE>
static hipError_t launch_generic(int route, const void* x, void* y, int64_t rows, int64_t width, int64_t ow,
                                 const int32_t* hq, int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    using OutT = typename OutTraits<STAGE>::T;
    const int64_t n_out = rows * ow;
    const int64_t blocks = (n_out + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    hipError_t e = hipSuccess;
    std::lock_guard<std::mutex> hold(cext::g_tab_mu);  // until the launch is enqueued
    if (route == FIR_CDECIM_GENERIC32) {
        const std::vector<uint32_t> pk = cext::pack_dot2(hq, L);
        const uint32_t* pd = (const uint32_t*)table_locked(pk.data(), sizeof(uint32_t) * pk.size(), s, &e);
        if (!pd) return e;
        return launch_recorded(route, 0, fir1d_cplx_decim_generic32_kernel<STAGE>, grid, 0, s, (const uint32_t*)x,
                               (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, pd, L, 32 - acc_bits, frac);
    }
    const int32_t* td = (const int32_t*)table_locked(hq, sizeof(int32_t) * 2 * (size_t)L, s, &e);
    if (!td) return e;
    if (route == FIR_CDECIM_GENERIC128)
        return launch_recorded(route, 0, fir1d_cplx_decim_generic_kernel<STAGE, true>, grid, 0, s, (const int16_t*)x,
                               (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, td, L, frac, acc_bits);
    return launch_recorded(route, 0, fir1d_cplx_decim_generic_kernel<STAGE, false>, grid, 0, s, (const int16_t*)x,
                           (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, td, L, frac, acc_bits);
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
            return launch_generic<st>(route, x, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits, stream);
        });
    if (e != hipSuccess) return *err = std::string("fir1d cplx decim launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace cdecim
