// cext_launch.h — the host side that the kernel sources of the complex-tap rate-changing FIRs
// share (fir1d_cplx_decim.hip, fir1d_cplx_interp.hip, fir1d_cplx_resample.hip,
// fir1d_cplx_stream.hip, fir1d_cplx_rstream.hip): the common head of
// check(), the exactness tests behind the routes, the generic-32 tap packing, the launch record,
// the generic kernels' tap-table cache and launch, and the host halves of the decimating tile kernel
// of cdecim and cstream and of the resampling tile kernel of cresample and crstream.  No library compiles this directory on its own; each includes this header
// into its one kernel source.  The device code they share is in cext_device.h.
//
// Everything here has internal linkage (an unnamed namespace, `static`): the libraries are loaded
// into one process and each keeps its own launch record and table cache.  Nothing `inline` with
// external linkage may be added: it would become one weak dynamic symbol common to all of them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "cext_device.h"
#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_hip.h"

namespace cext {
namespace {

// csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its order and its texts
// (tests/test_cabi_c*.py hold them against libfir_hip.so's).  A library's check() starts with this
// and goes on with its own rate and size checks.
static int check_head(int64_t rows, int64_t width, const int32_t* hq, int L, int frac, int acc_bits, int stage,
                      std::string* err) {
    if (stage != FIR_OUT_U8_SAT && stage != FIR_OUT_I32)
        return *err = "out_stage must be FIR_OUT_U8_SAT or FIR_OUT_I32", FIR_EINVAL;
    if (rows < 0 || width < 0) return *err = "rows and width must be >= 0", FIR_EINVAL;
    if (!hq) return *err = "hq must not be NULL", FIR_EINVAL;
    if (L < 1 || L > FIR_MAX_TAPS) return *err = "taps must be in [1, " + std::to_string(FIR_MAX_TAPS) + "]", FIR_EINVAL;
    if (frac < 1 || acc_bits < 1) return *err = "frac_bits and acc_bits must be >= 1", FIR_EINVAL;
    return FIR_OK;
}

// 32-bit wrap-around sums over v_dot2_i32_i16 are exact for the call: both tap parts (and -hi) fit
// in int16, and the wrap and the rounding shift stay inside 32 bits
static bool dot2_ok(const int32_t* hq, int L, int frac, int acc_bits) {
    if (acc_bits > 32 || frac > 31) return false;
    for (int64_t k = 0; k < 2 * (int64_t)L; ++k)
        if (hq[k] < -32767 || hq[k] > 32767) return false;
    return true;
}

// csrc/fir1d.hip's needs_wide for int16 samples over the 2 L tap parts: a no-wrap call whose exact
// sum could reach 2^63
static bool needs_wide(const int32_t* hq, int L, int acc_bits) {
    if (acc_bits < 64) return false;
    unsigned __int128 habs = 0;
    for (int64_t k = 0; k < 2 * (int64_t)L; ++k) habs += (unsigned __int128)(hq[k] < 0 ? -(int64_t)hq[k] : (int64_t)hq[k]);
    return habs * 32768 >= ((unsigned __int128)1 << 63);
}

// The generic-32 kernels' table: pk[2k] = (hr[k], -hi[k]), pk[2k + 1] = (hi[k], hr[k]), int16 pairs
static std::vector<uint32_t> pack_dot2(const int32_t* hq, int L) {
    std::vector<uint32_t> pk(2 * (size_t)L);
    for (int k = 0; k < L; ++k) {
        const uint32_t r16 = (uint32_t)hq[2 * k] & 0xFFFFu, i16 = (uint32_t)hq[2 * k + 1] & 0xFFFFu;
        pk[2 * (size_t)k] = r16 | (((uint32_t)(-hq[2 * k + 1]) & 0xFFFFu) << 16);
        pk[2 * (size_t)k + 1] = i16 | (r16 << 16);
    }
    return pk;
}

// ---- the launch wrapper: every kernel of a library is launched here, and what was launched is
// kept for last_launch (this thread).  0 is every library's FIR_*_NONE.
thread_local int t_route = 0, t_bucket = 0;

// a call that passed its checks: nothing launched yet
static void launch_none() {
    t_route = 0;
    t_bucket = 0;
}

template <typename... KArgs, typename... Args>
static hipError_t launch_recorded(int route, int bucket, void (*kernel)(KArgs...), dim3 grid, size_t shmem,
                                  hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(fir::kBlock), shmem, s, (KArgs)args...);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        t_route = route;
        t_bucket = bucket;
    }
    return e;
}

static void last_launch(int* route, int* bucket) {
    if (route) *route = t_route;
    if (bucket) *bucket = t_bucket;
}

// ---- the generic kernels' tap tables: device copies cached per device by the exact bytes they
// hold, confirmed by comparing them, uploaded once (complete before the call returns).  A caller
// holds g_tab_mu from the lookup until its launch is enqueued, so when the cached bytes of a
// device pass kTabCap a device-wide synchronise leaves no launch that reads a table outstanding
// and the device's tables are freed; a table used inside a stream capture is never freed (the
// graph may replay it), and nothing is evicted while a capture is under way.
constexpr size_t kTabCap = size_t(64) << 20;
struct Table {
    int dev;
    std::vector<uint8_t> key;
    void* d;
    bool pinned;
};
static std::mutex g_tab_mu;
static std::vector<Table> g_tabs;

static const void* table_locked(const void* host, size_t bytes, hipStream_t s, hipError_t* e) {
    int dev = 0;
    if ((*e = hipGetDevice(&dev)) != hipSuccess) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    size_t held = 0;
    for (Table& t : g_tabs) {
        if (t.dev != dev) continue;
        if (t.key.size() == bytes && std::memcmp(t.key.data(), host, bytes) == 0) {
            t.pinned |= capturing;
            return t.d;
        }
        held += t.key.size();
    }
    if (held && held + bytes > kTabCap && !capturing && hipDeviceSynchronize() == hipSuccess) {
        for (size_t i = g_tabs.size(); i-- > 0;)
            if (g_tabs[i].dev == dev && !g_tabs[i].pinned) {
                (void)hipFree(g_tabs[i].d);
                g_tabs.erase(g_tabs.begin() + (ptrdiff_t)i);
            }
    }
    void* d = nullptr;
    if ((*e = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
    if ((*e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    const uint8_t* hb = (const uint8_t*)host;
    g_tabs.push_back(Table{dev, std::vector<uint8_t>(hb, hb + bytes), d, false});
    return d;
}

// ---- the launch of a library's generic kernels: k32 its 32-bit kernel (route r32, over the packed
// table), k64 and k128 the exact ones (r128: the 128-bit sums; over hq itself).  go(kernel, grid,
// table, t0, t1) launches `kernel` through launch_recorded with the library's own arguments, the
// device table and the two trailing ints: (shl, frac) of k32, (frac, acc_bits) of the others.
template <typename K32, typename K64, typename Go>
static hipError_t launch_generic(int route, int r32, int r128, K32 k32, K64 k64, K64 k128, int64_t n_out,
                                 const int32_t* hq, int L, int frac, int acc_bits, hipStream_t s, Go go) {
    const int64_t blocks = (n_out + fir::kBlock - 1) / fir::kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    hipError_t e = hipSuccess;
    std::lock_guard<std::mutex> hold(g_tab_mu);  // until the launch is enqueued
    if (route == r32) {
        const std::vector<uint32_t> pk = pack_dot2(hq, L);
        const void* pd = table_locked(pk.data(), sizeof(uint32_t) * pk.size(), s, &e);
        return pd ? go(k32, grid, pd, 32 - acc_bits, frac) : e;
    }
    const void* td = table_locked(hq, sizeof(int32_t) * 2 * (size_t)L, s, &e);
    return td ? go(route == r128 ? k128 : k64, grid, td, frac, acc_bits) : e;
}

// ---- the host half of cext_device.h's decimating tile kernel (cdecim, cstream).

// -1 for a bad decim / phase / width
static int64_t decim_out_width(int64_t width, int decim, int phase) {
    if (width < 0 || decim < 1 || phase < 0 || phase >= decim) return -1;
    return width > phase ? (width - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

static int tile_bucket_of(int L) {
    for (const int b : kTileBuckets)
        if (L <= b) return b;
    return kTileMaxTaps;
}

// The geometry a call needs for the tile kernel (the exactness test, dot2_ok, is the caller's).
// Sets the tap bucket when it holds.
static bool tile_route_ok(uintptr_t x, int64_t rows, int64_t width, int64_t ow, int L, int decim, int stage, int* bucket) {
    if (decim < 2 || decim > kTileMaxD || L > kTileMaxTaps || stage != FIR_OUT_I32 || x % 16 != 0 ||
        (rows != 1 && width % kChunk != 0))  // every row starts as x does
        return false;
    const int64_t tiles = (ow + kTileT - 1) / kTileT;
    // the grid is at most rows * tiles < 2^31 workgroups; the kernel holds a tile index in 32 bits
    if (!(width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / tiles)) return false;
    *bucket = tile_bucket_of(L);
    return true;
}

// go(IntTag<LP>) for the bucket LP
template <typename Go>
static hipError_t with_tile_bucket(int bucket, Go go) {
    switch (bucket) {
        case 2: return go(fir::IntTag<2>{});
        case 4: return go(fir::IntTag<4>{});
        case 6: return go(fir::IntTag<6>{});
        case 8: return go(fir::IntTag<8>{});
        case 12: return go(fir::IntTag<12>{});
        case 16: return go(fir::IntTag<16>{});
        case 24: return go(fir::IntTag<24>{});
        case 32: return go(fir::IntTag<32>{});
        case 48: return go(fir::IntTag<48>{});
        default: return go(fir::IntTag<kTileMaxTaps>{});
    }
}

// the taps in window order, zero-padded to LP
template <int LP>
static TileTaps<LP> pack_window_taps(const int32_t* hq, int L) {
    TileTaps<LP> t;
    for (int p = 0; p < LP; ++p) {
        const int32_t hr = p < L ? hq[2 * (L - 1 - p)] : 0, hi = p < L ? hq[2 * (L - 1 - p) + 1] : 0;
        const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
        t.a[p] = r16 | (ni16 << 16);
        t.b[p] = i16 | (r16 << 16);
    }
    return t;
}

// the launch geometry of bucket LP at decimation D
struct TileGeom {
    int G, PL;  // tiles per workgroup, dwords per plane
    uint32_t magic, groups;
    size_t lds;
    dim3 grid;
};
static TileGeom tile_geom(int D, int LP, int64_t rows, int64_t ow) {
    TileGeom g;
    g.G = tile_tiles_per_group(D);
    g.PL = (tile_chunks(kChunk - 1, g.G, D, LP) * kChunk + D - 1) / D;
    g.magic = (1u << kMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (ow + (int64_t)g.G * kTileT - 1) / ((int64_t)g.G * kTileT);
    g.groups = (uint32_t)groups;
    g.lds = (size_t)D * g.PL * sizeof(uint32_t);
    g.grid = dim3((unsigned)(rows * groups));
    return g;
}

// ---- the host half of cext_device.h's resampling tile kernel (cresample, crstream).

// The U windows of a period.  Phase q: p the first tap, c the frame (from the period's first) that
// tap meets, n the taps, k0 the first dword of its window counted from S, the first frame of the
// lowest window; need: the longest sub-filter; kmax: the highest k0.
struct RsPlan {
    int S = 0, need = 0, kmax = 0;
    int p[kRsMaxUD] = {}, c[kRsMaxUD] = {}, n[kRsMaxUD] = {}, k0[kRsMaxUD] = {};
};

// centre: the filter's shift in intermediate frames, L / 2 for the one-shot entry and 0 for the
// causal streaming one.  With centre = 0, c >= 0 and n - 1 <= (L - 1) / U, so S >= -((L - 1) / U);
// c <= D - 1 and n >= need - 1, so k0 <= D.
static RsPlan rs_plan_of(int L, int U, int D, int phase, int centre) {
    RsPlan pl;
    int lo = 0;
    bool any = false;
    for (int q = 0; q < U; ++q) {
        const int a = phase + centre + q * D;
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

static int rs_bucket_of(int need) {
    for (const int b : kRsBuckets)
        if (need <= b) return b;
    return kRsMaxNP;
}

// go(IntTag<NP>) for the bucket NP
template <typename Go>
static hipError_t with_rs_bucket(int bucket, Go go) {
    switch (bucket) {
        case 1: return go(fir::IntTag<1>{});
        case 2: return go(fir::IntTag<2>{});
        case 3: return go(fir::IntTag<3>{});
        case 4: return go(fir::IntTag<4>{});
        case 6: return go(fir::IntTag<6>{});
        case 8: return go(fir::IntTag<8>{});
        case 10: return go(fir::IntTag<10>{});
        case 12: return go(fir::IntTag<12>{});
        case 16: return go(fir::IntTag<16>{});
        case 20: return go(fir::IntTag<20>{});
        case 24: return go(fir::IntTag<24>{});
        case 28: return go(fir::IntTag<28>{});
        default: return go(fir::IntTag<kRsMaxNP>{});
    }
}

// the launch geometry of bucket NP at the rates U / D under a plan
struct RsGeom {
    int P, T, ext, PL;  // periods per workgroup and per tile, window dwords a period can read, dwords per plane
    uint32_t magic, groups;
    size_t lds;
    dim3 grid;
};

// The geometry and the tap, window and offset tables of a launch; false (never taken: rs_slots
// bounds U * NP, kRsMaxExt the windows) when the plan does not fit the tables.
template <int NP>
static bool rs_setup(const int32_t* hq, int U, int D, const RsPlan& pl, int64_t rows, int64_t ow, RsGeom* g,
                     ResampleTaps<NP>* t) {
    g->P = rs_periods(D);
    g->ext = pl.kmax + NP;
    const int chunks = rs_chunks(kChunk - 1, g->P, D, g->ext);  // lead <= 3
    if (U * NP > rs_slots(NP) || g->ext > kRsOffs || chunks > kRsMaxIt * fir::kBlock) return false;
    g->PL = (chunks * kChunk + D - 1) / D;
    for (int k = 0; k < kRsOffs; ++k) t->off[k] = (uint32_t)((k % D) * g->PL + k / D);
    for (int q = 0; q < U; ++q) {
        t->k0[q] = (uint32_t)pl.k0[q];
        for (int w = 0; w < pl.n[q]; ++w) {  // window dword w is frame S + k0 + w = c - (n - 1 - w): tap n - 1 - w
            const int k = pl.p[q] + U * (pl.n[q] - 1 - w);
            const int32_t hr = hq[2 * k], hi = hq[2 * k + 1];
            const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
            t->a[q * NP + w] = r16 | (ni16 << 16);
            t->b[q * NP + w] = i16 | (r16 << 16);
        }
    }
    // periods per tile: the workgroup's periods, halved while the tile's outputs exceed kRsOutBytes
    g->T = g->P;
    while (g->T > kRsMinT && g->T * U * 8 > kRsOutBytes) g->T /= 2;
    const int in_dwords = (D * g->PL + 3) & ~3;
    const uint32_t stage_bytes = (uint32_t)(g->T * U * 8) + 16u;
    g->lds = (size_t)in_dwords * sizeof(uint32_t) + phys(stage_bytes) + 4;
    g->magic = (1u << kMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (ow + (int64_t)g->P * U - 1) / ((int64_t)g->P * U);
    g->groups = (uint32_t)groups;
    g->grid = dim3((unsigned)(rows * groups));
    return true;
}

}  // namespace
}  // namespace cext
