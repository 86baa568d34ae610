// fir1d_cplx.hip — the complex-coefficient 1-D fixed-point FIR for complex int16.
//
//   x: rows x width frames of interleaved int16 (xr, xi); hq: L x 2 int32 (hr[k], hi[k]); c = L / 2
//
//   re[n] = stage(round(wrap_acc( sum_k hr[k] * xr[n-k+c] - hi[k] * xi[n-k+c] )))
//   im[n] = stage(round(wrap_acc( sum_k hr[k] * xi[n-k+c] + hi[k] * xr[n-k+c] )))
//
// Frames outside a row are zero; each sum is one exact integer sum of its 2 L products, wrapped
// once to acc_bits; round and stage as in fir1d_lds.hip.  With every hi[k] = 0 the call IS
// launch_fir1d_rows with channels = 2 and the taps hr (forwarded, so bit for bit).  Two kernels:
//
//  * fir1d_cplx_kernel — the hot path (cplx_path_ok).  One interleaved frame is one dword, and
//    v_dot2_i32_i16 of that dword against the packed pair A[k] = (hr, -hi) is the real part of
//    one tap's product, against B[k] = (hi, hr) the imaginary part: two v_dot2 per tap and output
//    frame, no permute and no v_alignbit (every window element is a whole dword).  The frames of
//    all rows are one flat stream, as in fir1d_lds.hip.  A workgroup owns kCxTile = 1024
//    consecutive frames and stages them plus kCxPadL = 32 frames before and kCxPadR = 36 after
//    (the LP - 1 halo frames and the slack of the last 16-byte row read) in LDS as dwords: one
//    16-byte global load per thread for the tile, one dword each for the 68 halo frames, zero
//    outside [0, rows * width).  Lane u owns the V = kCxVec = 4 consecutive output frames 4u .. 4u
//    + 3 of the tile and reads the V + LP - 1 window dwords behind them back as whole 16-byte LDS
//    rows (the window start floored to a 16-byte row: OFF dwords of lead).  With V = 4 the lanes
//    of a ds_read_b128 are 16 bytes apart, so each of its 16-lane groups covers every one of the
//    64 banks exactly once: conflict free (V = 8 would put them 32 bytes apart, two-way).  Then
//    2 LP v_dot2 per output frame (wrap-around, no clamp) over the two tap tables passed BY VALUE
//    in the kernel arguments (read with scalar loads; no device table, nothing allocated, so the
//    call can be captured in a graph).  Filters are zero-padded to a bucket length LP in
//    {2, 4, 6, 8, 12, 16, 24, 32, 48, 64}, shifted by LP/2 - L/2 so the centre frame stays where
//    it was.  The accumulators are 32-bit wrap-around, exact mod 2^32, which is all the wrap to
//    acc_bits <= 32 needs (shl/ashr, skipped at 32: ACC32); rounding is fir_common.h's
//    overflow-free form.
//    Rows: with more than one row, rows are a multiple of 4 frames, so a lane's 4 outputs never
//    straddle two rows; a lane whose window crosses a row edge zeroes the other row's frames
//    before its MACs (a branch few waves take: one in eight at 4096-frame rows).
//    Output: a lane's 4 (re, im) int32 pairs are 32 bytes, so per-lane stores would leave the
//    lanes of one store instruction 32 bytes apart (the form the register kernel measured 6 %
//    slow, profiles/r01).  A whole wave's 256 frames (2 KiB) go through a wave-private LDS stage
//    instead and out as two runs of 64 consecutive 16-byte vectors (1 KiB per store instruction,
//    non-temporal: y is written once and not read here).  These are direct 16-byte stores, so the
//    fast path needs y 16-byte aligned (x too, for the staging loads).  The partial wave at the
//    end of the stream stores per lane, the last partial vector element by element.
//    LDS per workgroup: 4368 B of window + 8192 B of output stage = 12.3 KiB.  Registers: the
//    largest instantiation (LP = 64) holds 72 window dwords and 8 results; none spills
//    (profiles/cplx/resource_usage.txt: the -Rpass-analysis=kernel-resource-usage report of every
//    instantiation).
//
//  * fir1d_cplx_generic_kernel — every other legal call (int32-sized taps or a -32768 part, more
//    than 64 taps, acc_bits > 32, frac_bits > 31, the u8 stage, an x or y that is not 16-byte
//    aligned, rows of 4k + 2 or odd frames): one output frame per thread, walking the taps
//    whose frame lies in the row, taps from a cached device table, exact 64-bit sums (128-bit when
//    needs_wide says so for the 2 L tap parts).  Where only the tap count, an alignment, the row
//    length or the stage keeps a call off the fast path (int16-sized parts, acc_bits <= 32,
//    frac_bits <= 31, x 4-byte aligned) the same walk runs on 32-bit wrap-around accumulators with
//    two v_dot2 per tap over a packed device table (fir1d_cplx_generic32_kernel): the 64-bit form
//    took 185 us for 2^22 frames at 65 taps, 2.5 times the two-real-filter composition
//    (profiles/cplx).  Untuned beyond that.
#include <string>
#include <type_traits>
#include <vector>

#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_launch.h"

namespace fir {

constexpr int kCxMaxTaps = 64;
constexpr int kCxVec = 4;                                  // output frames per lane
constexpr int kCxTile = kBlock * kCxVec;                   // output frames per workgroup
constexpr int kCxPadL = 32;                                // LDS frames before the tile (>= HLE, a multiple of 4)
constexpr int kCxPadR = 36;                                // ... after it: the right halo (<= 32) and read slack (<= 3)
constexpr int kCxSpan = kCxPadL + kCxTile + kCxPadR;

typedef uint32_t cx_u4 __attribute__((ext_vector_type(4)));

template <int LP>
struct TapsCx {
    uint32_t a[LP];  // window frame m meets tap h'[LP-1-m]: a[m] = (hr, -hi), the real part's pair
    uint32_t b[LP];  //                                      b[m] = (hi, hr), the imaginary part's
};

template <int LP, bool ACC32>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_kernel(const uint32_t* __restrict__ x, int32_t* __restrict__ y,
                                                            int64_t total, int64_t rowlen, TapsCx<LP> taps, int shl,
                                                            int frac) {
    constexpr int HLE = LP - 1 - LP / 2;                  // frames left of an output
    constexpr int HRE = LP / 2;
    constexpr int OFF = (kCxPadL - HLE) % 4;              // window start inside its 16-byte LDS row
    constexpr int NQ = (OFF + kCxVec + LP - 1 + 3) / 4;   // 16-byte LDS rows per lane
    constexpr int ND = NQ * 4;                            // window dwords
    static_assert(HLE <= kCxPadL && HRE + 3 <= kCxPadR && kCxPadL % 4 == 0, "halo exceeds the LDS padding");
    static_assert(kCxPadL - HLE - OFF + (kBlock - 1) * kCxVec + ND <= kCxSpan, "window read past the LDS span");
    __shared__ __attribute__((aligned(16))) uint32_t win[kCxSpan];
    __shared__ cx_u4 sout[kBlock / kWave][kWave * kCxVec * 2 / 4];

    const int64_t t0 = (int64_t)blockIdx.x * kCxTile;     // first output frame of this workgroup
    const int64_t o0 = t0 + (int64_t)threadIdx.x * kCxVec;  // ... of this lane
    // ---- stage frames [t0 - kCxPadL, t0 + kCxTile + kCxPadR) (zero outside [0, total))
    if (o0 + kCxVec <= total) {
        *reinterpret_cast<cx_u4*>(&win[kCxPadL + threadIdx.x * kCxVec]) = *reinterpret_cast<const cx_u4*>(x + o0);
    } else {
        uint32_t v[kCxVec];
#pragma unroll
        for (int j = 0; j < kCxVec; ++j) v[j] = o0 + j < total ? x[o0 + j] : 0u;
#pragma unroll
        for (int j = 0; j < kCxVec; ++j) win[kCxPadL + threadIdx.x * kCxVec + j] = v[j];
    }
    if (threadIdx.x < kCxPadL + kCxPadR) {  // the halos, one frame per thread
        const int i = threadIdx.x;
        const int li = i < kCxPadL ? i : kCxTile + i;
        const int64_t gi = t0 - kCxPadL + li;
        win[li] = gi >= 0 && gi < total ? x[gi] : 0u;
    }
    __syncthreads();
    if (o0 >= total) return;

    // ---- the lane's window: frames [o0 - HLE - OFF, ...)
    uint32_t d[ND];
    {
        const cx_u4* src = reinterpret_cast<const cx_u4*>(&win[kCxPadL + threadIdx.x * kCxVec - HLE - OFF]);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const cx_u4 r = src[q];
            d[4 * q] = r.x;
            d[4 * q + 1] = r.y;
            d[4 * q + 2] = r.z;
            d[4 * q + 3] = r.w;
        }
    }
    if (rowlen > 0) {  // more than one row: zero the frames of a neighbouring row
        const int64_t col0 = o0 % rowlen;
        if (col0 < HLE || col0 + kCxVec + HRE > rowlen) {
            const int64_t ws = o0 - HLE - OFF;  // global frame of window dword 0
            const int64_t rs = o0 - col0;       // this row's first frame (the lane's outputs stay in it)
            const int lo = (int)max((int64_t)-1, min(rs - ws, (int64_t)ND));
            const int hi = (int)max((int64_t)-1, min(rs + rowlen - ws, (int64_t)ND));
#pragma unroll
            for (int q = 0; q < ND; ++q)
                if (!(q >= lo && q < hi)) d[q] = 0u;
        }
    }
    uint32_t qo[2 * kCxVec];
#pragma unroll
    for (int j = 0; j < kCxVec; ++j) {
        uint32_t re = 0, im = 0;
#pragma unroll
        for (int m = 0; m < LP; ++m) {
            re = dot2_acc(d[OFF + j + m], taps.a[m], re);
            im = dot2_acc(d[OFF + j + m], taps.b[m], im);
        }
        qo[2 * j] = (uint32_t)round_acc<ACC32>(re, shl, frac);
        qo[2 * j + 1] = (uint32_t)round_acc<ACC32>(im, shl, frac);
    }

    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wo = o0 - lane * kCxVec;       // the wave's first output frame
    if (wo + kWave * kCxVec <= total) {          // wave-uniform: the wave's 2 KiB as two 1 KiB runs
        cx_u4* wb = sout[threadIdx.x >> 6];
        wb[2 * lane] = cx_u4{qo[0], qo[1], qo[2], qo[3]};
        wb[2 * lane + 1] = cx_u4{qo[4], qo[5], qo[6], qo[7]};
        __builtin_amdgcn_wave_barrier();  // one wave's LDS ops complete in order
        asm volatile("" ::: "memory");
        cx_u4* dst = reinterpret_cast<cx_u4*>(y + 2 * wo);
#pragma unroll
        for (int r = 0; r < 2; ++r) __builtin_nontemporal_store(wb[r * kWave + lane], &dst[r * kWave + lane]);
        return;
    }
    if (o0 + kCxVec <= total) {
        cx_u4* dst = reinterpret_cast<cx_u4*>(y + 2 * o0);
        dst[0] = cx_u4{qo[0], qo[1], qo[2], qo[3]};
        dst[1] = cx_u4{qo[4], qo[5], qo[6], qo[7]};
    } else {
#pragma unroll
        for (int j = 0; j < kCxVec; ++j)
            if (o0 + j < total) {
                y[2 * (o0 + j)] = (int32_t)qo[2 * j];
                y[2 * (o0 + j) + 1] = (int32_t)qo[2 * j + 1];
            }
    }
}

// One output frame per thread: frame gi = r * width + n sums the taps k whose frame n - k + c
// lies in row r (the in-row test as loop bounds); taps[2k] = hr[k], taps[2k + 1] = hi[k].
template <int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_generic_kernel(const int16_t* __restrict__ x,
                                                                    typename OutTraits<STAGE>::T* __restrict__ y,
                                                                    int64_t total, int64_t width,
                                                                    const int32_t* __restrict__ taps, int L, int frac,
                                                                    int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= total) return;
    const int64_t n = gi % width, r = gi / width;
    const int64_t c = L / 2;
    // 0 <= n - k + c < width  <=>  n + c - width < k <= n + c
    const int64_t k_lo = n + c - width + 1 > 0 ? n + c - width + 1 : 0;
    const int64_t k_hi = n + c < L - 1 ? n + c : L - 1;
    const int16_t* __restrict__ xr = x + 2 * r * width;
    using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
    using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;
    Acc re = 0, im = 0;
    for (int64_t k = k_lo; k <= k_hi; ++k) {
        const int64_t hr = taps[2 * k], hi = taps[2 * k + 1];
        const int64_t f = n - k + c;
        const int64_t ar = xr[2 * f], ai = xr[2 * f + 1];
        re += (Acc)(SAcc)(hr * ar) - (Acc)(SAcc)(hi * ai);
        im += (Acc)(SAcc)(hr * ai) + (Acc)(SAcc)(hi * ar);
    }
    if constexpr (WIDE) {
        y[2 * gi] = stage_out128<STAGE>(round128((__int128)re, frac, acc_bits));
        y[2 * gi + 1] = stage_out128<STAGE>(round128((__int128)im, frac, acc_bits));
    } else {
        y[2 * gi] = stage_out<STAGE>(round64((int64_t)re, frac, acc_bits));
        y[2 * gi + 1] = stage_out<STAGE>(round64((int64_t)im, frac, acc_bits));
    }
}

// The same walk on 32-bit wrap-around accumulators, for calls off the fast path only by their tap
// count, alignment, row length or stage: both tap parts within [-32767, 32767], acc_bits <= 32,
// frac <= 31, x 4-byte aligned (a frame is then one aligned dword).  pk[2k] = (hr[k], -hi[k]),
// pk[2k + 1] = (hi[k], hr[k]): two v_dot2_i32_i16 per tap, as in the fast kernel.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void fir1d_cplx_generic32_kernel(const uint32_t* __restrict__ x,
                                                                      typename OutTraits<STAGE>::T* __restrict__ y,
                                                                      int64_t total, int64_t width,
                                                                      const uint32_t* __restrict__ pk, int L, int shl,
                                                                      int frac) {
    const int64_t b0 = (int64_t)blockIdx.x * kBlock;
    const int64_t gi = b0 + threadIdx.x;
    if (gi >= total) return;
    const int64_t n = gi % width, r = gi / width;
    const int64_t c = L / 2;
    const uint32_t* __restrict__ xf = x + r * width + n + c;  // tap k meets frame xf[-k]
    uint32_t re = 0, im = 0;
    // A workgroup whose 256 frames and all their windows lie inside one row (known from its first
    // frame, so the same for every lane) walks all L taps without a test: the loop is wave-uniform
    // and its taps come by scalar loads.  At a row's ends each lane walks the taps its row meets.
    const int64_t bn = b0 % width;
    if (bn + c - (L - 1) >= 0 && bn + kBlock - 1 + c < width) {
#pragma unroll 4
        for (int k = 0; k < L; ++k) {
            const uint32_t d = xf[-(int64_t)k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
    } else {
        const int64_t k_lo = n + c - width + 1 > 0 ? n + c - width + 1 : 0;
        const int64_t k_hi = n + c < L - 1 ? n + c : L - 1;
        for (int64_t k = k_lo; k <= k_hi; ++k) {
            const uint32_t d = xf[-k];
            re = dot2_acc(d, pk[2 * k], re);
            im = dot2_acc(d, pk[2 * k + 1], im);
        }
    }
    y[2 * gi] = stage_out32<STAGE>(round32(re, shl, frac));
    y[2 * gi + 1] = stage_out32<STAGE>(round32(im, shl, frac));
}

// ---------------------------------------------------------------------------------------
// Host side.

int check_fir1d_cplx(int64_t rows, int64_t width, const int32_t* hq, int L, int frac, int acc_bits, int stage,
                     std::string* err) {
    const int rc = check_fir1d(FIR_IN_I16, rows, width, 2, hq, L, 1, frac, acc_bits, stage, err);
    if (rc) return rc;
    int64_t rw = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || rw > INT64_MAX / 8)
        return *err = "rows * width * 2 * 4 bytes must fit in int64", FIR_EINVAL;
    return FIR_OK;
}

// 32-bit wrap-around sums over v_dot2_i32_i16 are exact for the call: both tap parts (and -hi) fit
// in int16, and the wrap and the rounding shift stay inside 32 bits
static bool cplx_dot2_ok(const int32_t* hq, int L, int frac, int acc_bits) {
    if (acc_bits > 32 || frac > 31) return false;
    for (int64_t k = 0; k < 2 * (int64_t)L; ++k)
        if (hq[k] < -32767 || hq[k] > 32767) return false;
    return true;
}

bool cplx_path_ok(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int frac,
                  int acc_bits, int stage) {
    if (L > kCxMaxTaps || stage != FIR_OUT_I32 || !cplx_dot2_ok(hq, L, frac, acc_bits)) return false;
    if ((uintptr_t)x % 16 != 0 || (uintptr_t)y % 16 != 0) return false;
    if (!(rows == 1 || width % kCxVec == 0)) return false;  // a lane's 4 outputs never straddle two rows
    return rows * width < ((int64_t)1 << 40);               // the grid: rows * width / 1024 workgroups
}

template <int LP>
static hipError_t launch_cplx_lp(const void* x, void* y, int64_t total, int64_t rowlen, const int32_t* hq, int L,
                                 int frac, int acc_bits, hipStream_t s) {
    // zero-padded taps h'[dsh + k] = h[k], dsh = LP/2 - L/2: the centre frame does not move
    int32_t hr[LP] = {}, hi[LP] = {};
    const int dsh = LP / 2 - L / 2;
    for (int k = 0; k < L; ++k) {
        hr[dsh + k] = hq[2 * k];
        hi[dsh + k] = hq[2 * k + 1];
    }
    TapsCx<LP> t;
    for (int m = 0; m < LP; ++m) {
        const uint32_t r16 = (uint32_t)hr[LP - 1 - m] & 0xFFFFu, i16 = (uint32_t)hi[LP - 1 - m] & 0xFFFFu;
        const uint32_t ni16 = (uint32_t)(-hi[LP - 1 - m]) & 0xFFFFu;
        t.a[m] = r16 | (ni16 << 16);
        t.b[m] = i16 | (r16 << 16);
    }
    const unsigned blocks = (unsigned)((total + kCxTile - 1) / kCxTile);
    if (acc_bits == 32)
        FIR_LAUNCH((fir1d_cplx_kernel<LP, true>), dim3(blocks), dim3(kBlock), 0, s, (const uint32_t*)x,
                           (int32_t*)y, total, rowlen, t, 0, frac);
    else
        FIR_LAUNCH((fir1d_cplx_kernel<LP, false>), dim3(blocks), dim3(kBlock), 0, s, (const uint32_t*)x,
                           (int32_t*)y, total, rowlen, t, 32 - acc_bits, frac);
    return hipGetLastError();
}

static hipError_t launch_cplx_fast(const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L,
                                   int frac, int acc_bits, hipStream_t s) {
    const int64_t total = rows * width, rl = rows > 1 ? width : 0;
    const auto go = [&](auto lp) {
        return launch_cplx_lp<decltype(lp)::value>(x, y, total, rl, hq, L, frac, acc_bits, s);
    };
    if (L <= 2) return go(IntTag<2>{});
    if (L <= 4) return go(IntTag<4>{});
    if (L <= 6) return go(IntTag<6>{});
    if (L <= 8) return go(IntTag<8>{});
    if (L <= 12) return go(IntTag<12>{});
    if (L <= 16) return go(IntTag<16>{});
    if (L <= 24) return go(IntTag<24>{});
    if (L <= 32) return go(IntTag<32>{});
    if (L <= 48) return go(IntTag<48>{});
    return go(IntTag<kCxMaxTaps>{});
}

template <int STAGE>
static hipError_t launch_cplx_generic(const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L,
                                      int frac, int acc_bits, hipStream_t s) {
    using OutT = typename OutTraits<STAGE>::T;
    const int64_t total = rows * width;
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    std::string err;
    if ((uintptr_t)x % 4 == 0 && cplx_dot2_ok(hq, L, frac, acc_bits)) {
        std::vector<uint32_t> pk(2 * (size_t)L);
        for (int k = 0; k < L; ++k) {
            const uint32_t r16 = (uint32_t)hq[2 * k] & 0xFFFFu, i16 = (uint32_t)hq[2 * k + 1] & 0xFFFFu;
            pk[2 * (size_t)k] = r16 | (((uint32_t)(-hq[2 * k + 1]) & 0xFFFFu) << 16);
            pk[2 * (size_t)k + 1] = i16 | (r16 << 16);
        }
        const uint32_t* pd = (const uint32_t*)device_table(pk.data(), sizeof(uint32_t) * pk.size(), &err);
        if (!pd) return hipErrorOutOfMemory;
        TableHold hold(pd, s);
        FIR_LAUNCH((fir1d_cplx_generic32_kernel<STAGE>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const uint32_t*)x, (OutT*)y, total, width, pd, L, 32 - acc_bits, frac);
        return hipGetLastError();
    }
    const int32_t* td = (const int32_t*)device_table(hq, sizeof(int32_t) * 2 * (size_t)L, &err);
    if (!td) return hipErrorOutOfMemory;
    TableHold hold(td, s);
    if (needs_wide(FIR_IN_I16, hq, 2 * L, acc_bits))
        FIR_LAUNCH((fir1d_cplx_generic_kernel<STAGE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const int16_t*)x, (OutT*)y, total, width, td, L, frac, acc_bits);
    else
        FIR_LAUNCH((fir1d_cplx_generic_kernel<STAGE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const int16_t*)x, (OutT*)y, total, width, td, L, frac, acc_bits);
    return hipGetLastError();
}

int launch_fir1d_cplx(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int frac, int acc_bits,
                      int stage, void* y, hipStream_t stream, std::string* err) {
    const int rc = check_fir1d_cplx(rows, width, hq, L, frac, acc_bits, stage, err);
    if (rc) return rc;
    if (rows == 0 || width == 0) return FIR_OK;
    if (!x || !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    bool real = true;
    for (int k = 0; k < L; ++k) real &= hq[2 * k + 1] == 0;
    if (real) {  // real taps: the two channels filtered independently with hr
        std::vector<int32_t> hr((size_t)L);
        for (int k = 0; k < L; ++k) hr[k] = hq[2 * k];
        return launch_fir1d_rows(x, FIR_IN_I16, rows, width, 2, hr.data(), L, frac, acc_bits, stage, y, stream, err);
    }
    hipError_t e;
    if (cplx_path_ok(x, y, rows, width, hq, L, frac, acc_bits, stage))
        e = launch_cplx_fast(x, y, rows, width, hq, L, frac, acc_bits, stream);
    else
        e = with_stage(stage, [&](auto st) {
            return launch_cplx_generic<st>(x, y, rows, width, hq, L, frac, acc_bits, stream);
        });
    if (e != hipSuccess) return *err = std::string("fir1d cplx launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace fir
