// cext_device.h — the device side that the kernel sources of the complex-tap rate-changing FIRs
// share (fir1d_cplx_decim.hip, fir1d_cplx_interp.hip, fir1d_cplx_resample.hip,
// fir1d_cplx_stream.hip, fir1d_cplx_rstream.hip): input staging, the polyphase LDS planes, the LDS
// output stage, the decimating tile kernel body of cdecim and cstream, the resampling tile kernel
// body of cresample and crstream, and the steps of the generic kernels.
//
// Everything here is a constexpr, a plain struct or a __device__ __forceinline__ function of
// internal linkage.  No __global__ kernel lives here: the libraries are loaded into one process, and
// a kernel template of a shared namespace would give them one weak host stub in common (the rule at
// the top of cext_launch.h).  Each library keeps its kernels, under its own names, in its own
// namespace; where a body lives here the kernel is a wrapper that passes its arguments on.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fir_common.h"

namespace cext {
namespace {

using fir::dot2_acc;
using fir::kBlock;
using fir::OutTraits;

constexpr int kChunk = 4;  // frames per staging step of one thread (16 bytes): a fast route's row unit
// a / D == (a * (2^18 / D + 1)) >> 18 for a < 2^14 and 2 <= D <= 16, the product staying below 2^31 + 2^14
constexpr int kMagicShift = 18;

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2_a4 __attribute__((ext_vector_type(2), aligned(4)));  // a store at int32 alignment

// ---- input staging of the fast kernels.  One interleaved frame is one dword.  A workgroup stages
// nchunks 16-byte chunks of its row from frame o on (a multiple of 4, so every chunk is aligned as
// x is), thread t the chunks t, t + 256, ...: first every load of the thread (at most MAXIT), then
// the LDS writes.

// The load phase.  edge(f) is frame f of the row for a chunk that is not wholly inside [0, width);
// the kernel passes a lambda that captures BY REFERENCE: a functor that holds copies of xr and
// width costs the tile kernel two VGPRs (hipcc no longer folds the four frames' range tests).
template <int MAXIT, typename Edge>
__device__ __forceinline__ void stage_load(u4 (&raw)[MAXIT], const uint32_t* __restrict__ xr, int64_t o, int nchunks,
                                           int64_t width, Edge edge) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kChunk;
        if (f >= 0 && f + kChunk <= width) {
            raw[it] = *reinterpret_cast<const u4*>(xr + f);
        } else {  // a chunk that crosses a row end, or lies outside the row
#pragma unroll
            for (int j = 0; j < kChunk; ++j) raw[it][j] = edge(f + j);
        }
    }
}

// The LDS writes into D polyphase planes of PL dwords: staged frame a, counted from frame o + skip
// (the up to 3 frames before it are dropped), goes to plane a mod D, index a / D.  A lane that reads
// frames D apart then reads consecutive dwords of one plane: conflict free for every D.
template <int MAXIT>
__device__ __forceinline__ void scatter_planes(uint32_t* __restrict__ lds, const u4 (&raw)[MAXIT], int nchunks, int skip,
                                               int D, int PL, uint32_t magic) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            const int ai = kChunk * k + i - skip;
            if (ai < 0) continue;
            const uint32_t a = (uint32_t)ai;
            // every factor is below 2^24: v_mul_u32_u24 (full rate) instead of v_mul_lo_u32
            const uint32_t idx = (uint32_t)__umul24(a, magic) >> kMagicShift;  // a / D
            const uint32_t pl = a - (uint32_t)__umul24(idx, (uint32_t)D);      // a % D
            lds[(uint32_t)__umul24(pl, (uint32_t)PL) + idx] = raw[it][i];
        }
    }
}

// ---- the LDS output stage of the interpolating kernels: logical byte b of a tile's output run
// lives at b + 4 * (b / 128), one pad dword per 32
__host__ __device__ constexpr uint32_t phys(uint32_t b) { return b + ((b >> 7) << 2); }

// The run [sh, end) of the stage goes to y (yt: the run's first byte, sh = yt mod 16) as 16-byte
// vectors at 16-byte addresses, consecutive lanes consecutive vectors; the partial vector at either
// end of the run dword by dword, inside the run's own bytes.
__device__ __forceinline__ void write_run(const uint32_t* __restrict__ outw, char* yt, uint32_t sh, uint32_t end) {
    const uint32_t nvec = (end + 15u) >> 4;
    for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) {
        const uint32_t lo = 16u * v;
        if (lo >= sh && lo + 16u <= end) {
            u4 q;
            q.x = outw[phys(lo) >> 2];
            q.y = outw[phys(lo + 4) >> 2];
            q.z = outw[phys(lo + 8) >> 2];
            q.w = outw[phys(lo + 12) >> 2];
            *reinterpret_cast<u4*>(yt - sh + lo) = q;
        } else {
            const uint32_t b0 = lo < sh ? sh : lo, b1 = lo + 16u < end ? lo + 16u : end;
            for (uint32_t b = b0; b < b1; b += 4u) *reinterpret_cast<uint32_t*>(yt - sh + b) = outw[phys(b) >> 2];
        }
    }
}

// ---- the decimating tile kernel: the hot path of cdecim (HIST = false) and cstream (HIST = true).
//
// v_dot2_i32_i16 of a frame against A = (hr, -hi) is the real part of one tap's product, against
// B = (hi, hr) the imaginary part: two v_dot2 per tap and KEPT frame on 32-bit wrap-around
// accumulators (exact mod 2^32, all the wrap to acc_bits <= 32 needs; ACC32 skips the wrap).  Every
// window element is a whole dword, so no D needs a v_alignbit.  The taps are reversed into window
// order and zero-padded at the window's far end to a bucket length LP in kTileBuckets; both tables
// travel BY VALUE in the kernel arguments (scalar loads; no device table, nothing allocated: the
// call can be captured in a graph).
//
// Tiling.  A tile is kTileT = 512 consecutive output frames of ONE row (never two rows, so frames
// outside the row are settled once, at staging).  A workgroup of 256 lanes owns G = max(1, 16 / D)
// consecutive tiles of its row and stages the (G * 512 - 1) * D + LP input frames behind them, from
// the 16-byte boundary at or below the first one (lead = 0..3 frames), with at most kTileMaxIt = 9
// loads per thread.  At most 8257 frames = 32.3 KiB of LDS: four workgroups per CU.  Grid: rows x
// groups.  Output m's window starts at frame m * D + base of its row; base is the library's.
//
// LDS layout.  Kept outputs are D dwords apart, so a linear window would put the lanes of a
// ds_read_b32 D dwords apart (a 16-way bank conflict at D = 16).  With scatter_planes, window dword
// p of output j of tile g is at plane (lead + p) mod D, index (lead + p) / D + 512 g + j: plane and
// index base are wave-uniform, and consecutive lanes read consecutive dwords.  Lane u owns outputs u
// and u + 256 of each tile (one ds_read_b32 each per window dword) and stores each as 8 bytes at
// int32 alignment, 512 contiguous bytes per wave, non-temporal (y is written once, not read here).
//
// The MAC loop takes the window in steps of tile_step(LP) <= 16 dwords: the step's 2 x 16 LDS reads
// are issued together, then its 4 x 16 v_dot2 run; the steps are a real loop with the taps indexed
// in the kernel arguments (still scalar loads), so the LDS, not the registers, sets the occupancy
// (the numbers: csrc_cdecim/fir1d_cplx_decim.hip).
constexpr int kTileT = 512;        // output frames per tile: 2 per lane
constexpr int kTileMaxD = 16;      // G * D <= kTileMaxD: tiles per workgroup G = max(1, 16 / D)
constexpr int kTileMaxTaps = 64;   // the largest tap bucket
constexpr int kTileBuckets[] = {2, 4, 6, 8, 12, 16, 24, 32, 48, kTileMaxTaps};

// 16-byte chunks a workgroup of G tiles stages: lead + the last window's start + LP frames
__host__ __device__ constexpr int tile_chunks(int lead, int G, int D, int LP) {
    return (lead + (G * kTileT - 1) * D + LP + kChunk - 1) / kChunk;
}
constexpr int tile_tiles_per_group(int D) { return D >= kTileMaxD ? 1 : kTileMaxD / D; }
constexpr int tile_max_chunks() {
    int m = 0;
    for (int D = 2; D <= kTileMaxD; ++D) {
        const int c = tile_chunks(kChunk - 1, tile_tiles_per_group(D), D, kTileMaxTaps);
        m = c > m ? c : m;
    }
    return m;
}
constexpr int kTileMaxIt = (tile_max_chunks() + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kTileMaxIt == 9, "staging steps");
static_assert(kChunk * tile_max_chunks() < (1 << 14), "the magic division's range");

// window dwords per step of the MAC loop: the whole window up to 16 taps, 12 or 16 of it beyond
constexpr int tile_step(int LP) { return LP <= 16 ? LP : (LP % 16 == 0 ? 16 : 12); }

template <int LP>
struct TileTaps {
    uint32_t a[LP];  // window frame p meets tap k = L - 1 - p (zero for p >= L): a[p] = (hr, -hi)
    uint32_t b[LP];  //                                                          b[p] = (hi, hr)
};

// hist: the first frame of the rows x H frames of history, or NULL for a zero one (HIST only)
template <int LP, bool ACC32, bool HIST>
__device__ __forceinline__ void decim_tile(const uint32_t* __restrict__ x, const uint32_t* __restrict__ hist,
                                           int32_t* __restrict__ y, int64_t width, int64_t out_width, uint32_t groups,
                                           int G, int D, int base, int H, int PL, uint32_t magic,
                                           const TileTaps<LP>& taps, int shl, int frac) {
    constexpr int PB = tile_step(LP);
    static_assert(LP % PB == 0, "whole steps");
    extern __shared__ __attribute__((aligned(16))) uint32_t tile_lds[];  // D planes of PL dwords
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t m0 = (int64_t)tb * G * kTileT;   // first output frame of the workgroup
    const int64_t left = (out_width - m0 + kTileT - 1) / kTileT;
    const int gt = left < G ? (int)left : G;       // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = m0 * D + base;              // its first window's first frame in the row (< 0: outside, or history)
    const int64_t o = a0 & ~(int64_t)(kChunk - 1);  // LDS origin: floor to 4 frames
    const int lead = (int)(a0 - o);                // 0..3
    const int nchunks = tile_chunks(lead, gt, D, LP);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row
    u4 raw[kTileMaxIt];
    if constexpr (HIST) {  // frames [-H, 0) are the row's history (zero for a NULL one)
        stage_load(raw, xr, o, nchunks, width, [&](int64_t f) {
            const uint32_t* __restrict__ hr = hist ? hist + r * H + H : nullptr;  // frame f < 0 is hr[f]
            if (f >= 0) return f < width ? xr[f] : 0u;
            return hr && f >= -(int64_t)H ? hr[f] : 0u;
        });
    } else {
        stage_load(raw, xr, o, nchunks, width, [&](int64_t f) { return f >= 0 && f < width ? xr[f] : 0u; });
    }
    scatter_planes(tile_lds, raw, nchunks, 0, D, PL, magic);
    __syncthreads();

    // ---- lane u: outputs u and u + 256 of each tile g; tile g's windows are 512 g plane rows on
    const int u = threadIdx.x;
    const uint32_t idx0 = ((uint32_t)lead * magic) >> kMagicShift;
    const uint32_t pl0 = (uint32_t)lead - idx0 * (uint32_t)D;
    const uint32_t wrap = (uint32_t)D * PL - 1;
    for (int g = 0; g < gt; ++g) {
        uint32_t re0 = 0, im0 = 0, re1 = 0, im1 = 0;
        uint32_t pl = pl0, off = pl0 * PL + idx0 + g * kTileT;  // wave-uniform: the plane and pl * PL + index
        // tile_step(LP) window dwords at a time: first the step's reads, then its MACs
#pragma unroll 1
        for (int pb = 0; pb < LP; pb += PB) {
            uint32_t d0[PB], d1[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                d0[q] = tile_lds[off + u];
                d1[q] = tile_lds[off + u + kTileT / 2];
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
        const int64_t m = m0 + (int64_t)g * kTileT + u;
        int32_t* yo = y + (r * out_width + m) * 2;
        if (m < out_width)  // false only in the row's last tile
            __builtin_nontemporal_store(u2_a4{(uint32_t)fir::round_acc<ACC32>(re0, shl, frac),
                                              (uint32_t)fir::round_acc<ACC32>(im0, shl, frac)},
                                        reinterpret_cast<u2_a4*>(yo));
        if (m + kTileT / 2 < out_width)
            __builtin_nontemporal_store(u2_a4{(uint32_t)fir::round_acc<ACC32>(re1, shl, frac),
                                              (uint32_t)fir::round_acc<ACC32>(im1, shl, frac)},
                                        reinterpret_cast<u2_a4*>(yo + 2 * (kTileT / 2)));
    }
}

// ---- the resampling tile kernel: the hot path of cresample (HIST = false) and crstream (HIST = true).
//
// The decimator's input side, the interpolator's output side and the complex MAC; the work split,
// the D input planes, the by-value tap, window and offset tables and the LDS output stage are
// described at the top of csrc_cresample/fir1d_cplx_resample.hip.  What the two libraries differ in
// is the library's: S, the first frame of a period's lowest window (centred for the one-shot entry,
// causal and >= -H for the streaming one), and with HIST the frames [-H, 0) of a row, which staging
// takes from the row's history as decim_tile does.
constexpr int kRsInBytes = 4096;    // input bytes a workgroup keeps in flight, at least
constexpr int kRsMinT = 256;        // the smallest tile and workgroup: one pass, one period per lane
constexpr int kRsOutBytes = 16384;  // T = P halved while T * U * 8 exceeds this
constexpr int kRsMaxUD = 16;        // 2 <= U, D <= 16
constexpr int kRsMaxTaps = 128;
constexpr int kRsMaxNP = 32;        // the largest tap bucket: ceil(L / U) of the fast path
constexpr int kRsOffs = 64;         // window dwords a lane can address: the highest k0 + NP is 17 + 32

// periods per workgroup
__host__ __device__ constexpr int rs_periods(int D) {
    int P = kRsMinT;
    while (P * D * 4 < kRsInBytes) P *= 2;
    return P;
}
// 16-byte chunks a workgroup of n periods stages: lead + the last period's first frame + ext, the
// frames from there to the end of the furthest window (the highest k0 + NP)
__host__ __device__ constexpr int rs_chunks(int lead, int n, int D, int ext) {
    return (lead + (n - 1) * D + ext + kChunk - 1) / kChunk;
}
constexpr int kRsMaxExt = kRsMaxUD + 1 + kRsMaxNP;  // k0 <= D + 1
constexpr int rs_max_chunks() {
    int m = 0;
    for (int D = 2; D <= kRsMaxUD; ++D) {
        const int c = rs_chunks(kChunk - 1, rs_periods(D), D, kRsMaxExt);
        m = c > m ? c : m;
    }
    return m;
}
constexpr int kRsMaxIt = (rs_max_chunks() + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kRsMaxIt == 5, "staging steps");
static_assert(kChunk * kRsMaxIt * kBlock < (1 << 14), "the magic division's range");
static_assert(kRsMaxExt <= kRsOffs, "the offset table holds every window dword");

// the tap buckets, and the one below a bucket (0 below the first)
constexpr int kRsBuckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, kRsMaxNP};
constexpr int rs_prev_bucket(int NP) {
    int prev = 0;
    for (const int b : kRsBuckets) {
        if (b >= NP) break;
        prev = b;
    }
    return prev;
}
// Dwords per tap table of bucket NP: U * NP for the largest U that can land in it.  A longest
// sub-filter of more than prev taps has ceil(L / U) > prev, so L >= U * prev + 1 and, with L <= 128,
// U <= 127 / prev.
constexpr int rs_slots(int NP) {
    const int prev = rs_prev_bucket(NP);
    const int umax = prev < 1 || (kRsMaxTaps - 1) / prev > kRsMaxUD ? kRsMaxUD : (kRsMaxTaps - 1) / prev;
    return umax * NP;
}
static_assert(rs_slots(1) == 16 && rs_slots(16) == 160 && rs_slots(kRsMaxNP) == 128, "tap table sizes");

template <int NP>
struct ResampleTaps {
    uint32_t a[rs_slots(NP)];  // phase q, window dword w at q * NP + w: (hr, -hi) of the tap that meets it
    uint32_t b[rs_slots(NP)];  //                                        (hi, hr); zero where no tap does
    uint32_t k0[kRsMaxUD];     // phase q: its window's first dword, from the period's first window dword
    uint32_t off[kRsOffs];     // window dword k of a period lies (k mod D) * PL + k / D dwords from its plane row
};

// hist: the first frame of the rows x H frames of history, or NULL for a zero one (HIST only).
// taps is __restrict__: without it the NP = 32 kernels take 14 more SGPRs than with the body in the kernel.
template <int NP, bool ACC32, bool HIST>
__device__ __forceinline__ void resample_tile(const uint32_t* __restrict__ x, const uint32_t* __restrict__ hist,
                                              int32_t* __restrict__ y, int64_t width, int64_t out_width,
                                              uint32_t groups, int U, int D, int P, int T, int S, int ext, int H,
                                              int PL, uint32_t magic, const ResampleTaps<NP>& __restrict__ taps,
                                              int shl, int frac) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];  // D planes of PL dwords, then the output stage
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t v0 = (int64_t)tb * P;  // first period of the workgroup
    const int64_t m0 = v0 * U;           // ... and its first output frame
    const int TU = T * U;                // output frames per tile
    const int64_t left = (out_width - m0 + TU - 1) / TU;
    const int gt = left < P / T ? (int)left : P / T;  // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = v0 * D + S;                    // its first window's first frame (< 0: outside, or history)
    const int64_t o = a0 & ~(int64_t)(kChunk - 1);    // the first frame staged: floor to 4 frames
    const int lead = (int)(a0 - o);                   // 0..3
    const int nchunks = rs_chunks(lead, gt * T, D, ext);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row in D planes; LDS dword 0 is the first window's
    // first frame a0 (the up to 3 frames in front of it are never read)
    u4 raw[kRsMaxIt];
    if constexpr (HIST) {  // frames [-H, 0) are the row's history (zero for a NULL one)
        stage_load(raw, xr, o, nchunks, width, [&](int64_t f) {
            const uint32_t* __restrict__ hr = hist ? hist + r * H + H : nullptr;  // frame f < 0 is hr[f]
            if (f >= 0) return f < width ? xr[f] : 0u;
            return hr && f >= -(int64_t)H ? hr[f] : 0u;
        });
    } else {  // zero outside [0, width)
        stage_load(raw, xr, o, nchunks, width, [&](int64_t f) { return f >= 0 && f < width ? xr[f] : 0u; });
    }
    scatter_planes(rs_lds, raw, nchunks, lead, D, PL, magic);
    __syncthreads();

    uint32_t* const outw = rs_lds + ((D * PL + 3) & ~3);
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
                    for (int w = c * CW; w < (c + 1) * CW && w < NP; ++w) d[w - c * CW] = rs_lds[wrow + oo[w]];
#pragma unroll
                    for (int w = c * CW; w < (c + 1) * CW && w < NP; ++w) {
                        re = dot2_acc(d[w - c * CW], ta[w], re);
                        im = dot2_acc(d[w - c * CW], tq[w], im);
                    }
                }
                outw[phys(b) >> 2] = (uint32_t)fir::round_acc<ACC32>(re, shl, frac);
                outw[phys(b + 4u) >> 2] = (uint32_t)fir::round_acc<ACC32>(im, shl, frac);
            }
        }
        __syncthreads();

        // ---- the tile's output run [sh, end) of the stage, as 16-byte vectors at 16-byte addresses
        write_run(outw, yt, sh, sh + (uint32_t)no * 8u);
        __syncthreads();  // the next tile overwrites the stage
    }
}

// ---- the generic kernels: one output frame per thread, taps from a device table.

// the exact sums: 64 bits, or 128 when needs_wide says so
template <bool WIDE>
using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
template <bool WIDE>
using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;

// tap k, taps[2k] = hr[k] and taps[2k + 1] = hi[k], meets frame f of src
template <bool WIDE>
__device__ __forceinline__ void cmac(Acc<WIDE>& re, Acc<WIDE>& im, const int32_t* __restrict__ taps, int64_t k,
                                     const int16_t* __restrict__ src, int64_t f) {
    const int64_t hr = taps[2 * k], hi = taps[2 * k + 1];
    const int64_t ar = src[2 * f], ai = src[2 * f + 1];
    re += (Acc<WIDE>)(SAcc<WIDE>)(hr * ar) - (Acc<WIDE>)(SAcc<WIDE>)(hi * ai);
    im += (Acc<WIDE>)(SAcc<WIDE>)(hr * ai) + (Acc<WIDE>)(SAcc<WIDE>)(hi * ar);
}

// ... on 32-bit wrap-around accumulators: pk[2k] = (hr[k], -hi[k]), pk[2k + 1] = (hi[k], hr[k]),
// two v_dot2_i32_i16 per tap against the frame's dword d
template <typename K>
__device__ __forceinline__ void cmac32(uint32_t& re, uint32_t& im, const uint32_t* __restrict__ pk, K k, uint32_t d) {
    re = dot2_acc(d, pk[2 * k], re);
    im = dot2_acc(d, pk[2 * k + 1], im);
}

// round, stage and store output frame gi
template <int STAGE, bool WIDE>
__device__ __forceinline__ void store_frame(typename OutTraits<STAGE>::T* __restrict__ y, int64_t gi, Acc<WIDE> re,
                                            Acc<WIDE> im, int frac, int acc_bits) {
    if constexpr (WIDE) {
        y[2 * gi] = fir::stage_out128<STAGE>(fir::round128((__int128)re, frac, acc_bits));
        y[2 * gi + 1] = fir::stage_out128<STAGE>(fir::round128((__int128)im, frac, acc_bits));
    } else {
        y[2 * gi] = fir::stage_out<STAGE>(fir::round64((int64_t)re, frac, acc_bits));
        y[2 * gi + 1] = fir::stage_out<STAGE>(fir::round64((int64_t)im, frac, acc_bits));
    }
}

template <int STAGE>
__device__ __forceinline__ void store_frame32(typename OutTraits<STAGE>::T* __restrict__ y, int64_t gi, uint32_t re,
                                              uint32_t im, int shl, int frac) {
    y[2 * gi] = fir::stage_out32<STAGE>(fir::round32(re, shl, frac));
    y[2 * gi + 1] = fir::stage_out32<STAGE>(fir::round32(im, shl, frac));
}

// The polyphase walk of frame j = i * U + e of a row zero-stuffed by U: it meets the taps
// pe + U * t, tap t at frame n - t, for t in [t_lo, t_hi] (the taps whose frame lies in the row).
struct PolyWalk {
    int64_t pe, n, t_lo, t_hi;
};
__device__ __forceinline__ PolyWalk poly_walk(int64_t j, int64_t U, int L, int64_t width) {
    const int64_t i = j / U, e = j % U;
    PolyWalk w;
    w.pe = (e + L / 2) % U;
    w.n = i + (e + L / 2) / U;
    // 0 <= n - t < width  <=>  n - width < t <= n;  pe + U * t <= L - 1
    w.t_lo = w.n - width + 1 > 0 ? w.n - width + 1 : 0;
    const int64_t t_max = w.pe < L ? (L - 1 - w.pe) / U : -1;
    w.t_hi = w.n < t_max ? w.n : t_max;
    return w;
}

}  // namespace
}  // namespace cext
