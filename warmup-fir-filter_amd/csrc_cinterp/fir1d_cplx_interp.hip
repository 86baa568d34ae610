// fir1d_cplx_interp.hip — the interpolating complex-tap 1-D fixed-point FIR for complex int16:
// zero-stuff by U, then filter with complex taps, in one polyphase pass over x itself.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); c0 = L / 2
//   out_width = width * U;  output frame j = i*U + e (0 <= e < U) meets the taps p_e + U*t only,
//   p_e = (e + c0) mod U, c_e = (e + c0) div U, t = 0 .. n_e - 1 (n_e taps: p_e + U*t < L):
//   re[j] = stage(round(wrap_acc( sum_t hr[p_e+U*t] * xr[i+c_e-t] - hi[p_e+U*t] * xi[i+c_e-t] )))
//   im[j] = stage(round(wrap_acc( sum_t hr[p_e+U*t] * xi[i+c_e-t] + hi[p_e+U*t] * xr[i+c_e-t] )))
//
// The arithmetic is csrc/fir1d_cplx.hip's (frames outside a row are zero, one exact sum per part,
// wrapped once, overflow-free round-half-up, int32 or saturated-u8 stage), the tiling and the LDS
// output stage csrc/fir1d_interp.hip's.  This file is libfir_cinterp.so's own device side; it shares
// the header-only device helpers of csrc/ (fir_common.h, fir_dispatch.h) and of csrc_cext/
// (cext_device.h: the output-run writer, the generic kernels' steps) and nothing compiled from either.
//
//  * fir1d_cplx_interp_kernel — the hot path (FIR_CINTERP_FAST, see route_of).  One interleaved frame
//    is one dword, and v_dot2_i32_i16 of it against A = (hr, -hi) is the real part of one tap's
//    product, against B = (hi, hr) the imaginary part: two v_dot2 per sub-filter tap and output frame
//    on 32-bit wrap-around accumulators (exact mod 2^32, all the wrap to acc_bits <= 32 needs; ACC32
//    skips the wrap).
//
//    Work split.  A workgroup of 256 lanes owns kCiF = 2048 consecutive input frames of ONE row
//    (never two rows, so frames outside the row are zeroed once, at staging) and works through them
//    as tiles of T input frames, T = 2048 halved while the tile's T * U * 8 output bytes exceed
//    16 KiB, but not below 256 (T = 1024, 512, 512, 256 at U = 2, 3, 4, 5 and up).  A tile is computed
//    in passes of 256 frames: lane u owns input frame u of every pass and produces its U output
//    frames.  Grid: rows x ceil(width / 2048).
//
//    Input.  The workgroup stages the frames behind all of its outputs, from the 16-byte boundary at
//    or below the first one (lead = 0..3 frames), as dwords in a LINEAR LDS window: 16-byte global
//    loads, all of a thread's loads (at most kCiMaxIt = 3) issued before its first 16-byte LDS write.
//    p_e and c_e depend on e alone, so the window all U phases of a frame share is frames
//    [i + S, i + hi], S the least c_e - n_e + 1 and hi the greatest c_e: W = hi - S + 1 dwords,
//    ceil(L / U) or one more.  The lane reads the NP >= W dwords of its frame once per pass (lane
//    stride one dword: conflict free for ds_read_b32) and reuses them for every phase.  Every
//    element is a whole dword, so no phase needs a v_alignbit.  Taps: per phase the sub-filter in
//    window order, zero-padded to the bucket NP in {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 33}, as
//    two packed tables passed BY VALUE (read with scalar loads at the phase's offset inside a
//    run-time loop over e, so the registers do not depend on U): no device table, nothing
//    allocated, so the call can be captured in a graph.  ci_slots(NP) bounds U * NP for every (L, U)
//    that lands in a bucket: at most 176 dwords per table, 1.4 KiB of arguments.
//
//    Output.  The kernel is write dominated (8 U bytes out per 4 bytes in), and a lane's U output
//    frames are 8 U bytes from the next lane's.  Every result goes to an LDS output stage instead, at
//    the byte it has in the tile's output run, and the workgroup then writes that run as whole
//    16-byte vectors, consecutive lanes consecutive vectors (1 KiB per store instruction).  The stage
//    starts (y address mod 16) bytes in, so LDS vectors and global vectors line up for ANY int32 y
//    address and row length; the partial vector at either end of a tile goes out dword by dword,
//    inside the tile's own bytes.  Bank layout: byte b of the stage lives at b + 4 * (b / 128), one
//    pad dword per 32.  An (re, im) pair is stored as two ds_write_b32 (y may be only 4-byte aligned,
//    and the pad may part a pair), each with a lane stride of 2 U dwords: the 32 lanes of a write's
//    lane group span 2 U rows of 32 dwords, 16 / U lanes per row at banks 2 U apart, and each row is
//    one bank further on -- 2 U distinct offsets, so all 32 lanes hit distinct banks at U = 2, 4, 8
//    and 16 (at other U at most two lanes share a bank, which a ds_write_b32 absorbs).  The read-back
//    (four dwords per lane, lane stride four dwords, eight lanes per row) is conflict free as well.
//
//    LDS per workgroup: the window, (2048 + NP + 2) dwords rounded to chunks (at most 8.2 KiB), plus
//    T * U * 8 + 16 bytes of output stage with its padding: 16.5 KiB up to U = 4 and T * U * 8 = 2 KiB
//    * U beyond (33 KiB at U = 16): six workgroups per CU as a rule, three in the worst case.
//
//  * The generic kernels — every other legal call: one output frame per thread, walking the taps
//    k = p_e, p_e + U, ... whose frame lies in the row (the in-row test as loop bounds), taps from a
//    cached device table.  fir1d_cplx_interp_generic32_kernel (int16-sized parts, acc_bits <= 32,
//    frac <= 31, x 4-byte aligned): 32-bit wrap-around sums, two v_dot2 per tap over a packed (A, B)
//    table.  fir1d_cplx_interp_generic_kernel: exact 64-bit sums, or 128-bit when needs_wide says so.
#include <string>

#include "cinterp.h"
#include "cext_launch.h"
#include "fir_common.h"
#include "fir_dispatch.h"

namespace cinterp {

using cext::kChunk;  // frames per staging step of one thread (16 bytes)
using cext::launch_recorded;
using fir::dot2_acc;
using fir::IntTag;
using fir::kBlock;
using fir::OutTraits;

constexpr int kCiF = 2048;          // input frames per workgroup: G = kCiF / T tiles
constexpr int kCiMinT = 256;        // the smallest tile: one pass, one frame per lane
constexpr int kCiOutBytes = 16384;  // T = kCiF halved while T * U * 8 exceeds this
constexpr int kCiMaxU = 16;
constexpr int kCiMaxTaps = 128;
constexpr int kCiMaxPerPhase = 32;  // ceil(L / U) of the fast path
constexpr int kCiMaxNP = 33;        // the largest window bucket: ceil(L / U) + 1

// 16-byte chunks a workgroup stages: lead + its frames + the last frame's window (NP - 1 more)
__host__ __device__ constexpr int ci_chunks(int lead, int frames, int NP) {
    return (lead + frames + NP - 1 + kChunk - 1) / kChunk;
}
constexpr int kCiMaxIt = (ci_chunks(kChunk - 1, kCiF, kCiMaxNP) + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kCiMaxIt == 3, "staging steps");

// the window buckets, and the one below a bucket (0 below the first)
constexpr int kCiBuckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, kCiMaxNP};
constexpr int ci_prev_bucket(int NP) {
    int prev = 0;
    for (const int b : kCiBuckets) {
        if (b >= NP) break;
        prev = b;
    }
    return prev;
}
// Dwords per tap table of bucket NP: U * NP for the largest U that can land in it.  A window of
// W > prev dwords has ceil(L / U) >= W - 1 >= prev, so L > U * (prev - 1) and, with L <= 128,
// U <= 127 / (prev - 1).
constexpr int ci_slots(int NP) {
    const int prev = ci_prev_bucket(NP);
    const int umax = prev < 2 || (kCiMaxTaps - 1) / (prev - 1) > kCiMaxU ? kCiMaxU : (kCiMaxTaps - 1) / (prev - 1);
    return umax * NP;
}
static_assert(ci_slots(1) == 16 && ci_slots(16) == 176 && ci_slots(kCiMaxNP) == 132, "tap table sizes");

template <int NP>
struct TapsCi {
    uint32_t a[ci_slots(NP)];  // phase e, window dword w at e * NP + w: (hr, -hi) of the tap that meets it
    uint32_t b[ci_slots(NP)];  //                                        (hi, hr); zero where no tap does
};

template <int NP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_interp_kernel(const uint32_t* __restrict__ x,
                                                                   int32_t* __restrict__ y, int64_t width,
                                                                   uint32_t groups, int U, int T, int S, int PL,
                                                                   TapsCi<NP> taps, int shl, int frac) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ci_lds[];  // PL window dwords, then the output stage
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t i0 = (int64_t)tb * kCiF;  // first input frame of the workgroup
    const int64_t left = width - i0;
    const int nf = left < kCiF ? (int)left : kCiF;  // its frames (the row's last workgroup: fewer)
    const int gt = (nf + T - 1) / T;                // its tiles
    const int64_t a0 = i0 + S;                      // its first window's first frame (may be < 0)
    const int64_t o = a0 & ~(int64_t)(kChunk - 1);  // LDS origin: floor to 4 frames
    const int lead = (int)(a0 - o);                 // 0..3
    const int nchunks = ci_chunks(lead, nf, NP);
    const uint32_t* __restrict__ xr = x + r * width;

    // ---- stage frames [o, o + 4 * nchunks) of the row (zero outside [0, width)): first every load
    // of the thread, then the LDS writes.  The load loop is cext::stage_load's, kept as this
    // kernel's own text: through the helper hipcc allots the small buckets two VGPRs fewer.
    cext::u4 raw[kCiMaxIt];
#pragma unroll
    for (int it = 0; it < kCiMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kChunk;
        if (f >= 0 && f + kChunk <= width) {
            raw[it] = *reinterpret_cast<const cext::u4*>(xr + f);
        } else {  // a chunk that crosses a row end, or lies outside the row
            raw[it].x = f >= 0 && f < width ? xr[f] : 0u;
            raw[it].y = f + 1 >= 0 && f + 1 < width ? xr[f + 1] : 0u;
            raw[it].z = f + 2 >= 0 && f + 2 < width ? xr[f + 2] : 0u;
            raw[it].w = f + 3 >= 0 && f + 3 < width ? xr[f + 3] : 0u;
        }
    }
#pragma unroll
    for (int it = 0; it < kCiMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        *reinterpret_cast<cext::u4*>(ci_lds + kChunk * k) = raw[it];
    }
    __syncthreads();

    uint32_t* const outw = ci_lds + PL;
    const int u = threadIdx.x;
    const int64_t out_width = width * U;
    const uint32_t fstep = (uint32_t)U * 8u;  // bytes from an input frame's outputs to the next frame's
    for (int g = 0; g < gt; ++g) {
        const int64_t ig = i0 + (int64_t)g * T;                 // the tile's first input frame
        const int nv = width - ig < T ? (int)(width - ig) : T;  // its frames inside the row
        char* const yt = reinterpret_cast<char*>(y + (r * out_width + ig * U) * 2);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(yt) & 15u);  // the stage's first byte

        // ---- lane u: the U output frames of input frame u of every pass (kBlock frames), into the stage
        for (int fp = u; fp < nv; fp += kBlock) {
            uint32_t d[NP];
            const int wb = lead + g * T + fp;
#pragma unroll
            for (int w = 0; w < NP; ++w) d[w] = ci_lds[wb + w];
            uint32_t b = sh + (uint32_t)fp * fstep;  // frame fp, phase 0
            for (int e = 0; e < U; ++e, b += 8u) {
                const uint32_t* __restrict__ ta = taps.a + e * NP;  // wave-uniform
                const uint32_t* __restrict__ tq = taps.b + e * NP;
                uint32_t re = 0, im = 0;
                // at most 16 window dwords at a time, so that a phase's 2 NP tap dwords are never
                // all live in SGPRs at once (66 of them at NP = 33 spilled)
                constexpr int NC = (NP + 15) / 16, CW = (NP + NC - 1) / NC;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int w = c * CW; w < (c + 1) * CW && w < NP; ++w) {
                        re = dot2_acc(d[w], ta[w], re);
                        im = dot2_acc(d[w], tq[w], im);
                    }
                }
                outw[cext::phys(b) >> 2] = (uint32_t)fir::round_acc<ACC32>(re, shl, frac);
                outw[cext::phys(b + 4u) >> 2] = (uint32_t)fir::round_acc<ACC32>(im, shl, frac);
            }
        }
        __syncthreads();

        // ---- the tile's output run [sh, end) of the stage, as 16-byte vectors at 16-byte addresses
        cext::write_run(outw, yt, sh, sh + (uint32_t)nv * fstep);
        __syncthreads();  // the next tile overwrites the stage
    }
}

// One output frame per thread: frame gi = r * out_width + i * U + e sums the taps p_e + U * t whose
// frame i + c_e - t lies in row r; taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_interp_generic_kernel(const int16_t* __restrict__ x,
                                                                           typename OutTraits<STAGE>::T* __restrict__ y,
                                                                           int64_t n_out, int64_t width, int64_t U,
                                                                           const int32_t* __restrict__ taps, int L,
                                                                           int frac, int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t out_width = width * U;
    const int64_t j = gi % out_width, r = gi / out_width;
    const cext::PolyWalk w = cext::poly_walk(j, U, L, width);
    const int16_t* __restrict__ xr = x + 2 * r * width;
    cext::Acc<WIDE> re = 0, im = 0;
    for (int64_t t = w.t_lo; t <= w.t_hi; ++t) cext::cmac<WIDE>(re, im, taps, w.pe + U * t, xr, w.n - t);
    cext::store_frame<STAGE, WIDE>(y, gi, re, im, frac, acc_bits);
}

// The same walk on 32-bit wrap-around accumulators over the packed table; a frame is one aligned dword.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_interp_generic32_kernel(
    const uint32_t* __restrict__ x, typename OutTraits<STAGE>::T* __restrict__ y, int64_t n_out, int64_t width, int64_t U,
    const uint32_t* __restrict__ pk, int L, int shl, int frac) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t out_width = width * U;
    const int64_t j = gi % out_width, r = gi / out_width;
    const cext::PolyWalk w = cext::poly_walk(j, U, L, width);
    const uint32_t* __restrict__ xf = x + r * width + w.n;  // tap pe + U * t meets frame xf[-t]
    uint32_t re = 0, im = 0;
    for (int64_t t = w.t_lo; t <= w.t_hi; ++t) cext::cmac32(re, im, pk, w.pe + U * t, xf[-t]);
    cext::store_frame32<STAGE>(y, gi, re, im, shl, frac);
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t out_width(int64_t width, int up) {
    int64_t ow = 0;
    if (width < 0 || up < 1 || __builtin_mul_overflow(width, (int64_t)up, &ow)) return -1;
    return ow;
}

// csrc/fir1d.hip's check_fir1d for int16 of two channels and one filter, its order and its texts
// (tests/test_cabi_cinterp.py holds them against libfir_hip.so's), then the header's checks 2 to 4.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int frac,
          int acc_bits, int stage, std::string* err) {
    if (const int rc = cext::check_head(rows, width, hq, L, frac, acc_bits, stage, err)) return rc;
    if (up < 1) return *err = "up must be >= 1", FIR_EINVAL;
    int64_t rw = 0, n = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || __builtin_mul_overflow(rw, (int64_t)up, &n) || n > INT64_MAX / 8)
        return *err = "rows * width * up * 2 * 4 bytes must fit in int64", FIR_EINVAL;
    if (rows != 0 && width != 0 && (!x || !y)) return *err = "x and y must not be NULL", FIR_EINVAL;
    return FIR_OK;
}

// The window all U phases share: *S its first frame relative to the output's input frame, returns
// its dwords W = hi - S + 1 (the header's "window").
static int window_of(int L, int U, int* S) {
    int lo = 0, hi = 0;
    bool any = false;
    for (int e = 0; e < U; ++e) {
        const int pe = (e + L / 2) % U, ce = (e + L / 2) / U;
        if (pe >= L) continue;  // an empty phase: its outputs are 0
        const int ne = (L - pe + U - 1) / U;
        if (!any || ce - ne + 1 < lo) lo = ce - ne + 1;
        if (!any || ce > hi) hi = ce;
        any = true;
    }
    *S = lo;
    return hi - lo + 1;
}

static int bucket_of(int W) {
    for (const int b : kCiBuckets)
        if (W <= b) return b;
    return kCiMaxNP;
}

// input frames per tile: the workgroup's frames, halved while the tile's outputs exceed kCiOutBytes
static int tile_of(int U) {
    int T = kCiF;
    while (T > kCiMinT && T * U * 8 > kCiOutBytes) T /= 2;
    return T;
}

int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int frac,
             int acc_bits, int stage, int* bucket) {
    (void)y;  // y may sit at any element address on every route
    *bucket = 0;
    const bool d2 = cext::dot2_ok(hq, L, frac, acc_bits);
    if (d2 && up >= 2 && up <= kCiMaxU && L <= kCiMaxTaps && (L + up - 1) / up <= kCiMaxPerPhase &&
        stage == FIR_OUT_I32 && x % 16 == 0 && (rows == 1 || width % kChunk == 0)) {  // every row starts as x does
        const int64_t groups = (width + kCiF - 1) / kCiF;
        // the grid is rows * groups < 2^31 workgroups; the kernel holds a group index in 32 bits
        if (width < ((int64_t)1 << 40) && rows <= (((int64_t)1 << 31) - 1) / groups) {
            int S = 0;
            *bucket = bucket_of(window_of(L, up, &S));
            return FIR_CINTERP_FAST;
        }
    }
    if (d2 && x % 4 == 0) return FIR_CINTERP_GENERIC32;
    return cext::needs_wide(hq, L, acc_bits) ? FIR_CINTERP_GENERIC128 : FIR_CINTERP_GENERIC64;
}

// what the calling thread's last launch() launched: every kernel goes through cext::launch_recorded
void last_launch(int* route, int* bucket) { cext::last_launch(route, bucket); }

template <int NP>
static hipError_t launch_fast_np(const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int U,
                                 int S, int frac, int acc_bits, hipStream_t s) {
    if (U * NP > ci_slots(NP)) return hipErrorInvalidValue;  // ci_slots' bound: never taken
    TapsCi<NP> t = {};
    for (int e = 0; e < U; ++e) {
        const int pe = (e + L / 2) % U, ce = (e + L / 2) / U;
        const int ne = pe < L ? (L - pe + U - 1) / U : 0;
        for (int w = 0; w < NP; ++w) {  // window dword w is frame S + w: tap t = ce - S - w of the phase
            const int tt = ce - S - w;
            if (tt < 0 || tt >= ne) continue;
            const int32_t hr = hq[2 * (pe + U * tt)], hi = hq[2 * (pe + U * tt) + 1];
            const uint32_t r16 = (uint32_t)hr & 0xFFFFu, i16 = (uint32_t)hi & 0xFFFFu, ni16 = (uint32_t)(-hi) & 0xFFFFu;
            t.a[e * NP + w] = r16 | (ni16 << 16);
            t.b[e * NP + w] = i16 | (r16 << 16);
        }
    }
    const int T = tile_of(U);
    const int PL = ci_chunks(kChunk - 1, kCiF, NP) * kChunk;  // window dwords (lead <= 3)
    const uint32_t stage_bytes = (uint32_t)(T * U * 8) + 16u;
    const size_t lds = (size_t)PL * sizeof(uint32_t) + cext::phys(stage_bytes) + 4;
    const int64_t groups = (width + kCiF - 1) / kCiF;
    const dim3 grid((unsigned)(rows * groups));
    if (acc_bits == 32)
        return launch_recorded(FIR_CINTERP_FAST, NP, fir1d_cplx_interp_kernel<NP, true>, grid, lds, s, (const uint32_t*)x,
                               (int32_t*)y, width, (uint32_t)groups, U, T, S, PL, t, 0, frac);
    return launch_recorded(FIR_CINTERP_FAST, NP, fir1d_cplx_interp_kernel<NP, false>, grid, lds, s, (const uint32_t*)x,
                           (int32_t*)y, width, (uint32_t)groups, U, T, S, PL, t, 32 - acc_bits, frac);
}

static hipError_t launch_fast(int bucket, const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L,
                              int U, int frac, int acc_bits, hipStream_t s) {
    int S = 0;
    (void)window_of(L, U, &S);
    const auto go = [&](auto np) {
        return launch_fast_np<decltype(np)::value>(x, y, rows, width, hq, L, U, S, frac, acc_bits, s);
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
        default: return go(IntTag<kCiMaxNP>{});
    }
}

int launch(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int frac, int acc_bits,
           int stage, void* y, hipStream_t stream, std::string* err) {
    const int rc = check(x, y, rows, width, hq, L, up, frac, acc_bits, stage, err);
    if (rc) return rc;
    cext::launch_none();
    if (rows == 0 || width == 0) return FIR_OK;
    int bucket = 0;
    const int route = route_of((uintptr_t)x, (uintptr_t)y, rows, width, hq, L, up, frac, acc_bits, stage, &bucket);
    hipError_t e;
    if (route == FIR_CINTERP_FAST)
        e = launch_fast(bucket, x, y, rows, width, hq, L, up, frac, acc_bits, stream);
    else
        e = fir::with_stage(stage, [&](auto st) {
            return cext::launch_generic(
                route, FIR_CINTERP_GENERIC32, FIR_CINTERP_GENERIC128, fir1d_cplx_interp_generic32_kernel<st>,
                fir1d_cplx_interp_generic_kernel<st, false>, fir1d_cplx_interp_generic_kernel<st, true>, rows * width * up,
                hq, L, frac, acc_bits, stream, [&](auto kernel, dim3 grid, const void* table, int t0, int t1) {
                    return launch_recorded(route, 0, kernel, grid, 0, stream, x, y, rows * width * up, width, (int64_t)up,
                                           table, L, t0, t1);
                });
        });
    if (e != hipSuccess) return *err = std::string("fir1d cplx interp launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace cinterp
