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
// This file is the whole device side of libfir_cstream.so; it shares the header-only device helpers
// of csrc/ (fir_common.h, fir_dispatch.h) and nothing compiled from it.
//
//  * fir1d_cplx_stream_kernel — the hot path (FIR_CSTREAM_FAST, see route_of).  It is
//    csrc_cdecim/fir1d_cplx_decim.hip's fir1d_cplx_decim_kernel (read that header comment and
//    profiles/cdecim/README.md for the tiling, the D LDS planes, the magic division and why the MAC
//    loop is taken in steps of cd_step(LP) window dwords) with a causal window origin,
//    base = phase - (L - 1), and the row's history as one more argument.  Only the staging fallback
//    branch differs, the one for a 16-byte chunk that is not wholly inside [0, width): a frame f
//    with -H <= f < 0 is read from hist_in[r, H + f] (zero for a NULL history), a frame f < -H or
//    f >= width is zero.  A workgroup's first window starts at m0 * D + base >= -H, so only the up
//    to 3 frames of the 16-byte lead lie below -H.  The window's zero-padded far end (LP - L frames
//    past n) may fall past width: those frames are staged as zero and meet zero taps.  The 16-byte
//    branch, the LDS layout, the MAC loop and the 8-byte non-temporal stores are the decimator's.
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
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "cext_launch.h"
#include "cstream.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cstream {

using cext::dot2_ok;
using cext::launch_recorded;
using cext::needs_wide;
using cext::table_locked;
using fir::dot2_acc;
using fir::IntTag;
using fir::kBlock;
using fir::OutTraits;

constexpr int kCsT = 512;         // output frames per tile: 2 per lane
constexpr int kCsMaxD = 16;       // G * D <= kCsMaxD: tiles per workgroup G = max(1, 16 / D)
constexpr int kCsMaxTaps = 64;    // the largest tap bucket
constexpr int kCsChunk = 4;       // frames per staging step of one thread (16 bytes)
// a / D == (a * (2^18 / D + 1)) >> 18 for a < 2^14 and 2 <= D <= 16, the product staying below 2^31 + 2^14
constexpr int kCsMagicShift = 18;

// 16-byte chunks a workgroup of G tiles stages: lead + the last window's start + LP frames
__host__ __device__ constexpr int cs_chunks(int lead, int G, int D, int LP) {
    return (lead + (G * kCsT - 1) * D + LP + kCsChunk - 1) / kCsChunk;
}
constexpr int cs_tiles_per_group(int D) { return D >= kCsMaxD ? 1 : kCsMaxD / D; }
constexpr int cs_max_chunks() {
    int m = 0;
    for (int D = 2; D <= kCsMaxD; ++D) {
        const int c = cs_chunks(kCsChunk - 1, cs_tiles_per_group(D), D, kCsMaxTaps);
        m = c > m ? c : m;
    }
    return m;
}
constexpr int kCsMaxIt = (cs_max_chunks() + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kCsMaxIt == 9, "staging steps");
static_assert(kCsChunk * cs_max_chunks() < (1 << 14), "the magic division's range");

// window dwords per step of the MAC loop: the whole window up to 16 taps, 12 or 16 of it beyond
constexpr int cs_step(int LP) { return LP <= 16 ? LP : (LP % 16 == 0 ? 16 : 12); }

typedef uint32_t cs_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t cs_u2_a4 __attribute__((ext_vector_type(2), aligned(4)));  // a store at int32 alignment

template <int LP>
struct TapsCs {
    uint32_t a[LP];  // window frame p meets tap k = L - 1 - p (zero for p >= L): a[p] = (hr, -hi)
    uint32_t b[LP];  //                                                          b[p] = (hi, hr)
};

// hist: the first frame of hist_in (rows x H frames), or NULL for a zero history
template <int LP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_stream_kernel(const uint32_t* __restrict__ x,
                                                                   const uint32_t* __restrict__ hist,
                                                                   int32_t* __restrict__ y, int64_t width,
                                                                   int64_t out_width, uint32_t groups, int G, int D,
                                                                   int base, int H, int PL, uint32_t magic,
                                                                   TapsCs<LP> taps, int shl, int frac) {
    constexpr int PB = cs_step(LP);
    static_assert(LP % PB == 0, "whole steps");
    extern __shared__ __attribute__((aligned(16))) uint32_t cs_lds[];  // D planes of PL dwords
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t m0 = (int64_t)tb * G * kCsT;     // first output frame of the workgroup
    const int64_t left = (out_width - m0 + kCsT - 1) / kCsT;
    const int gt = left < G ? (int)left : G;       // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = m0 * D + base;              // its first window's first frame in the block (>= -H)
    const int64_t o = a0 & ~(int64_t)(kCsChunk - 1);  // LDS origin: floor to 4 frames
    const int lead = (int)(a0 - o);                // 0..3
    const int nchunks = cs_chunks(lead, gt, D, LP);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row's stream (the history below 0, zero below
    // -H and from width on): first every load of the thread, then the LDS writes
    uint32_t raw[kCsMaxIt][kCsChunk];
#pragma unroll
    for (int it = 0; it < kCsMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kCsChunk;
        if (f >= 0 && f + kCsChunk <= width) {
            const cs_u4 q = *reinterpret_cast<const cs_u4*>(xr + f);
            raw[it][0] = q.x;
            raw[it][1] = q.y;
            raw[it][2] = q.z;
            raw[it][3] = q.w;
        } else {  // a chunk that crosses the block's start or end, or lies outside the block
            const uint32_t* __restrict__ hr = hist ? hist + r * H + H : nullptr;  // frame f < 0 is hr[f]
#pragma unroll
            for (int j = 0; j < kCsChunk; ++j) {
                const int64_t fj = f + j;
                uint32_t v = 0u;
                if (fj >= 0) {
                    if (fj < width) v = xr[fj];
                } else if (hr && fj >= -(int64_t)H) {
                    v = hr[fj];
                }
                raw[it][j] = v;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < kCsMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
#pragma unroll
        for (int i = 0; i < kCsChunk; ++i) {
            const uint32_t a = (uint32_t)kCsChunk * (uint32_t)k + i;
            // every factor is below 2^24: v_mul_u32_u24 (full rate) instead of v_mul_lo_u32
            const uint32_t idx = (uint32_t)__umul24(a, magic) >> kCsMagicShift;  // a / D
            const uint32_t pl = a - (uint32_t)__umul24(idx, (uint32_t)D);        // a % D
            cs_lds[(uint32_t)__umul24(pl, (uint32_t)PL) + idx] = raw[it][i];
        }
    }
    __syncthreads();

    // ---- lane u: outputs u and u + 256 of each tile g; tile g's windows are 512 g plane rows on
    const int u = threadIdx.x;
    const uint32_t idx0 = ((uint32_t)lead * magic) >> kCsMagicShift;
    const uint32_t pl0 = (uint32_t)lead - idx0 * (uint32_t)D;
    const uint32_t wrap = (uint32_t)D * PL - 1;
    for (int g = 0; g < gt; ++g) {
        uint32_t re0 = 0, im0 = 0, re1 = 0, im1 = 0;
        uint32_t pl = pl0, off = pl0 * PL + idx0 + g * kCsT;  // wave-uniform: the plane and pl * PL + index
        // cs_step(LP) window dwords at a time: first the step's reads, then its MACs (header comment)
#pragma unroll 1
        for (int pb = 0; pb < LP; pb += PB) {
            uint32_t d0[PB], d1[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                d0[q] = cs_lds[off + u];
                d1[q] = cs_lds[off + u + kCsT / 2];
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
        const int64_t m = m0 + (int64_t)g * kCsT + u;
        int32_t* yo = y + (r * out_width + m) * 2;
        if (m < out_width)  // false only in the row's last tile
            __builtin_nontemporal_store(cs_u2_a4{(uint32_t)fir::round_acc<ACC32>(re0, shl, frac),
                                                 (uint32_t)fir::round_acc<ACC32>(im0, shl, frac)},
                                        reinterpret_cast<cs_u2_a4*>(yo));
        if (m + kCsT / 2 < out_width)
            __builtin_nontemporal_store(cs_u2_a4{(uint32_t)fir::round_acc<ACC32>(re1, shl, frac),
                                                 (uint32_t)fir::round_acc<ACC32>(im1, shl, frac)},
                                        reinterpret_cast<cs_u2_a4*>(yo + 2 * (kCsT / 2)));
    }
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
    using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
    using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;
    Acc re = 0, im = 0;
    for (int64_t k = 0; k <= k_hi; ++k) {
        const int64_t hr = taps[2 * k], hi = taps[2 * k + 1];
        const int64_t f = n - k;
        const int16_t* __restrict__ src = f >= 0 ? xr : hr_;
        const int64_t ar = src[2 * f], ai = src[2 * f + 1];
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
// (hi[k], hr[k]), two v_dot2_i32_i16 per tap; a frame is one aligned dword, of x or of the history.
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
        for (int k = 0; k < L; ++k) {
            const uint32_t d = xf[-(int64_t)k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
    } else {
        const int64_t k_x = n < H ? n : H;  // taps 0..k_x meet x, the rest the history
        for (int64_t k = 0; k <= k_x; ++k) {
            const uint32_t d = xf[-k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
        if (hist) {
            const uint32_t* __restrict__ hf = hist + r * H + H + n;  // frame n - k < 0 at hf[-k]
            for (int64_t k = k_x + 1; k <= H; ++k) {
                const uint32_t d = hf[-k];
                re = dot2_acc(d, pk[2 * k], re);
                im = dot2_acc(d, pk[2 * k + 1], im);
            }
        }
    }
    y[2 * gi] = fir::stage_out32<STAGE>(fir::round32(re, shl, frac));
    y[2 * gi + 1] = fir::stage_out32<STAGE>(fir::round32(im, shl, frac));
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

int64_t out_width(int64_t width, int decim, int phase) {
    if (width < 0 || decim < 1 || phase < 0 || phase >= decim) return -1;
    return width > phase ? (width - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

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

static int bucket_of(int L) {
    for (const int b : {2, 4, 6, 8, 12, 16, 24, 32, 48})
        if (L <= b) return b;
    return kCsMaxTaps;
}

int route_of(uintptr_t x, uintptr_t hist_in, uintptr_t y, uintptr_t hist_out, int64_t rows, int64_t width, int64_t ow,
             const int32_t* hq, int L, int decim, int frac, int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = dot2_ok(hq, L, frac, acc_bits);
    // a frame of a history is one dword to the 32-bit kernels (NULL and taps = 1: no history is read)
    const bool h4 = L == 1 || (hist_in % 4 == 0 && hist_out % 4 == 0);
    if (d2 && h4 && decim >= 2 && decim <= kCsMaxD && L <= kCsMaxTaps && stage == FIR_OUT_I32 && x % 16 == 0 &&
        (rows == 1 || width % kCsChunk == 0)) {  // every row starts as x does
        const int64_t tiles = (ow + kCsT - 1) / kCsT;
        // the grid is at most rows * tiles < 2^31 workgroups; the kernel holds a tile index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / tiles) {
            *bucket = bucket_of(L);
            return FIR_CSTREAM_FAST;
        }
    }
    if (d2 && h4 && x % 4 == 0) return FIR_CSTREAM_GENERIC32;
    return needs_wide(hq, L, acc_bits) ? FIR_CSTREAM_GENERIC128 : FIR_CSTREAM_GENERIC64;
}

// what the calling thread's last launch() launched as its FIR kernel: those go through
// cext::launch_recorded, the history kernel does not
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

template <int LP>
static hipError_t launch_fast_lp(const void* x, const void* hist, void* y, int64_t rows, int64_t width, int64_t ow,
                                 const int32_t* hq, int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    TapsCs<LP> t;
    for (int p = 0; p < LP; ++p) {
        const int32_t hr = p < L ? hq[2 * (L - 1 - p)] : 0, hi = p < L ? hq[2 * (L - 1 - p) + 1] : 0;
        const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
        t.a[p] = r16 | (ni16 << 16);
        t.b[p] = i16 | (r16 << 16);
    }
    const int base = phase - (L - 1);  // causal: output m's window starts at frame m * D + base of its row's stream
    const int G = cs_tiles_per_group(D);
    const int PL = (cs_chunks(kCsChunk - 1, G, D, LP) * kCsChunk + D - 1) / D;  // dwords per plane
    const uint32_t magic = (1u << kCsMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (ow + (int64_t)G * kCsT - 1) / ((int64_t)G * kCsT);
    const size_t lds = (size_t)D * PL * sizeof(uint32_t);
    const dim3 grid((unsigned)(rows * groups));
    if (acc_bits == 32)
        return launch_recorded(FIR_CSTREAM_FAST, LP, fir1d_cplx_stream_kernel<LP, true>, grid, lds, s,
                               (const uint32_t*)x, (const uint32_t*)hist, (int32_t*)y, width, ow, (uint32_t)groups, G, D,
                               base, L - 1, PL, magic, t, 0, frac);
    return launch_recorded(FIR_CSTREAM_FAST, LP, fir1d_cplx_stream_kernel<LP, false>, grid, lds, s, (const uint32_t*)x,
                           (const uint32_t*)hist, (int32_t*)y, width, ow, (uint32_t)groups, G, D, base, L - 1, PL, magic,
                           t, 32 - acc_bits, frac);
}

static hipError_t launch_fast(int bucket, const void* x, const void* hist, void* y, int64_t rows, int64_t width,
                              int64_t ow, const int32_t* hq, int L, int D, int phase, int frac, int acc_bits,
                              hipStream_t s) {
    const auto go = [&](auto lp) {
        return launch_fast_lp<decltype(lp)::value>(x, hist, y, rows, width, ow, hq, L, D, phase, frac, acc_bits, s);
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
        default: return go(IntTag<kCsMaxTaps>{});
    }
}

template <int STAGE>
static hipError_t launch_generic(int route, const void* x, const void* hist, void* y, int64_t rows, int64_t width,
                                 int64_t ow, const int32_t* hq, int L, int D, int phase, int frac, int acc_bits,
                                 hipStream_t s) {
    using OutT = typename OutTraits<STAGE>::T;
    const int64_t n_out = rows * ow;
    const int64_t blocks = (n_out + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    hipError_t e = hipSuccess;
    std::lock_guard<std::mutex> hold(cext::g_tab_mu);  // until the launch is enqueued
    if (route == FIR_CSTREAM_GENERIC32) {
        const std::vector<uint32_t> pk = cext::pack_dot2(hq, L);
        const uint32_t* pd = (const uint32_t*)table_locked(pk.data(), sizeof(uint32_t) * pk.size(), s, &e);
        if (!pd) return e;
        return launch_recorded(route, 0, fir1d_cplx_stream_generic32_kernel<STAGE>, grid, 0, s, (const uint32_t*)x,
                               (const uint32_t*)hist, (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, pd, L,
                               32 - acc_bits, frac);
    }
    const int32_t* td = (const int32_t*)table_locked(hq, sizeof(int32_t) * 2 * (size_t)L, s, &e);
    if (!td) return e;
    if (route == FIR_CSTREAM_GENERIC128)
        return launch_recorded(route, 0, fir1d_cplx_stream_generic_kernel<STAGE, true>, grid, 0, s, (const int16_t*)x,
                               (const int16_t*)hist, (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, td, L, frac,
                               acc_bits);
    return launch_recorded(route, 0, fir1d_cplx_stream_generic_kernel<STAGE, false>, grid, 0, s, (const int16_t*)x,
                           (const int16_t*)hist, (OutT*)y, n_out, width, ow, (int64_t)D, (int64_t)phase, td, L, frac,
                           acc_bits);
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
                return launch_generic<st>(route, x, hist_in, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits,
                                          stream);
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
