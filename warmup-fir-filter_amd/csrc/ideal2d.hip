// ideal2d.hip — float64 "ideal" model of the 2-D FIR (the fixed-vs-ideal check of fir_2d).
//
//   y[i,j] = acc after:  acc = +0.0
//                        for m in 0..R-1:            (outer, ascending)
//                          for n in 0..C-1:          (inner, ascending)
//                            acc = acc + h[m][n] * x[i - m + R/2][j - n + C/2]
//
// the 2-D extension of fir1d_ideal_rows (ideal.hip:1-9) with the centre rule of fir2d_fixed
// (fir2d.hip:3).  x uint8, h float64, y float64, no output clamp; samples outside the frame are
// zero; every product and every sum is rounded on its own (__dmul_rn / __dadd_rn, and the library
// is built with -ffp-contract=off).  The order of the additions is part of the contract (another
// order changes the bytes of most outputs), and so is the +0.0 start: a zero term is +-0.0, and
// +0.0 + -0.0 = +0.0, so the running sum is never -0.0 and adding the zero terms of the padding
// is identical to skipping them.  No f64 MFMA: its fused accumulate rounds once per term.
//
// fir2d_ideal_reg_kernel (R, C <= 5; x 4-byte aligned, y 16-byte aligned, whole dwords per row):
// the lane/DPP layout of the 1-D ideal kernel (ideal_reg.h).  A lane owns one dword (4 pixels)
// per input row, the (C-1)-pixel horizontal halo is one dword from each neighbouring lane by DPP
// wave shifts (lanes 0 / 63 load the seam dword), every sample is converted to f64 once per
// strip, and a wave's 256 outputs of a row go through LDS and out as two whole contiguous 1 KiB
// non-temporal rows.  Vertically a wave walks its strip top to bottom and keeps a RING OF R
// CONVERTED INPUT ROWS; each output row is formed completely, m-major and n-minor, when its last
// input row (row i + R/2, the m = 0 term) arrives: the row loaded m steps ago is the m term, so
// the sum runs in the contract's order.  (The fixed 2-D register kernel scatters each input row
// into a ring of partial outputs instead; an output then receives its rows in m-descending order,
// which is fine for integers and wrong here.)  Grid: (column tiles, strips, frames).
// fir2d_ideal_generic_kernel: one output per thread, any R x C (taps in HBM), any width and
// alignment, the same ordered sum, frames through blockIdx.z.
#include <algorithm>
#include <string>

#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_launch.h"

namespace fir {

template <int R, int C>
struct TapsIdeal2 {
    double h[R][C];
};

// Output rows per strip.  x is 1 of the 9 bytes per sample, so the R - 1 rows a strip re-reads
// cost (R - 1) / 16 / 9 < 3 % of the traffic; the height is bounded by nothing else (the ring
// holds R rows whatever it is), 16 keeps the grid of an 8192^2 frame at 4096 blocks.
constexpr int kIdeal2dStrip = 16;
// input rows loaded ahead of the row being summed = bodies of the unrolled row loop (see
// ideal2d_strip): the multiple of R that reaches 4.  4 frames of 8192^2, 3x3 / 5x5: 531 / 621 us
// with a lead of 2 rows -> 497 / 568 us (profiles/fir2d_ideal/); the multiple that reaches 8
// drops the register allocation to 4 / 2 waves per SIMD and doubles the code, and was not kept.
template <int R>
constexpr int kIdeal2dUnroll = R * ((4 + R - 1) / R);
constexpr int kIdeal2dMaxRC = 5;  // halo of at most 2 + 2 pixels: one neighbour dword each side

// One wave's strip.  FULL: all 256 columns of the wave lie in the frame (plain stores); otherwise
// lanes past the row end hold zeros (the right-hand padding) and their stores are masked.
// Nothing in the row loop branches around a memory instruction: every lane loads an in-frame
// dword of an in-frame row (column and row clamped, the value masked to zero where the clamp
// acted), so the loads of the rows ahead stay in flight, counted, behind the sums and stores of
// row t.  (Loads under `if`s made hipcc wait for vmcnt(0) right after issuing them, and with it
// for the previous row's stores: 534 / 684 us for 3x3 / 5x5, profiles/fir2d_ideal/.)
template <int R, int C, bool FULL>
__device__ __forceinline__ void ideal2d_strip(const uint8_t* __restrict__ x, double* __restrict__ y, int64_t H,
                                              int64_t W, const TapsIdeal2<R, C>& taps, int64_t cw, int lane,
                                              int64_t r0, int T,
                                              double __attribute__((ext_vector_type(2)))* wb) {
    constexpr int CC = C / 2, HLE = C - 1 - CC, HRE = CC;
    static_assert(HLE <= 4 && HRE <= 4, "halo must fit in one dword");
    constexpr int NS = HLE + 4 + HRE;
    constexpr int ABOVE = R - 1 - R / 2;  // input rows above an output row (the m = R-1 term)
    typedef double d2 __attribute__((ext_vector_type(2)));

    // W is a whole number of dwords (>= 1), so a lane's dword is in the row or past its end
    const int64_t c0 = cw + lane * 4;
    const bool own_ok = FULL || c0 < W;
    const uint32_t m_own = own_ok ? ~0u : 0u;
    const int64_t o_own = own_ok ? c0 : W - 4;
    // lanes 0 / 63 load the seam dword of the neighbouring wave tile (none at a frame edge: zero);
    // the other lanes' seam value is never used (DPP keeps it only where a lane has no source)
    int64_t o_seam = o_own;
    uint32_t m_seam = 0;
    if (lane == 0 && cw > 0) o_seam = cw - 4, m_seam = ~0u;
    if (lane == kWave - 1 && c0 + 4 < W) o_seam = c0 + 4, m_seam = ~0u;

    // step t handles input row r0 - ABOVE + t; rows outside the frame are zero
    auto load_raw = [&](int t, uint32_t& own, uint32_t& seam) {
        const int64_t r = r0 - ABOVE + t;
        const uint8_t* p = x + min(max(r, (int64_t)0), H - 1) * W;
        own = *reinterpret_cast<const uint32_t*>(p + o_own);
        seam = *reinterpret_cast<const uint32_t*>(p + o_seam);
    };
    auto convert = [&](int t, uint32_t own, uint32_t seam, double (&s)[NS]) {
        const int64_t r = r0 - ABOVE + t;
        const uint32_t mr = (r >= 0 && r < H) ? ~0u : 0u;  // wave-uniform
        own &= m_own & mr;
        seam &= m_seam & mr;
        uint32_t Wd[3];
        Wd[0] = from_prev_lane(seam, own);
        Wd[1] = own;
        Wd[2] = from_next_lane(seam, own);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int b = 4 - HLE + i;  // byte index in the 12-byte window
            s[i] = (double)((Wd[b / 4] >> (8 * (b % 4))) & 0xFFu);
        }
    };

    double ring[R][NS];  // slot t % R holds the converted window of the row of step t
    // Raw dwords of the UN rows ahead, slot t % UN: once the row of step t is converted its slot is
    // reloaded with the row of step t + UN.  Loads and stores share one in-order counter (vmcnt),
    // so waiting for a row's dwords also waits for every store issued before their load: UN rows
    // of lead leave UN rows of stores in flight per wave.  (A shorter lead, or a lead kept in
    // registers that are copied from step to step, makes every row wait for the previous row's
    // stores: a copy of a register has to wait for its load.)
    constexpr int UN = kIdeal2dUnroll<R>;  // a multiple of R: ring slot = (t % UN) % R
    uint32_t pa[UN], ps[UN];
#pragma unroll
    for (int d = 0; d < UN; ++d) load_raw(d, pa[d], ps[d]);
    int t = 0;
#pragma unroll
    for (int u = 0; u < R - 1; ++u) {  // the R - 1 rows before the first output row (T >= R)
        convert(t, pa[u], ps[u], ring[u]);
        load_raw(t + UN, pa[u], ps[u]);
        ++t;
    }
    for (;;) {
#pragma unroll
        for (int k = 0; k < UN; ++k) {  // unrolled: every slot index is a compile-time constant
            const int kk = (R - 1 + k) % UN, u = kk % R;
            convert(t, pa[kk], ps[kk], ring[u]);
            load_raw(t + UN, pa[kk], ps[kk]);  // (clamped past the strip's end: unused)
            // output row r0 + t - (R - 1): its m term is the row of step t - m
            double q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < R; ++m)
#pragma unroll
                    for (int n = 0; n < C; ++n)
                        acc = __dadd_rn(acc, __dmul_rn(taps.h[m][n], ring[(u - m + R) % R][HLE + j + CC - n]));
                q[j] = acc;
            }
            wb[lane * 2] = d2{q[0], q[1]};
            wb[lane * 2 + 1] = d2{q[2], q[3]};
            __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
            asm volatile("" ::: "memory");
            d2* yrow = reinterpret_cast<d2*>(y + (r0 + t - (R - 1)) * W + cw);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = i * kWave + lane;  // W is even: a 16-byte pair is in the row or past it
                if (FULL || cw + 2 * e < W) __builtin_nontemporal_store(wb[e], yrow + e);
            }
            __builtin_amdgcn_wave_barrier();  // the next row's LDS writes stay behind these reads
            asm volatile("" ::: "memory");
            if (++t == T) return;  // wave-uniform
        }
    }
}

template <int R, int C>
__global__ __launch_bounds__(kBlock) void fir2d_ideal_reg_kernel(const uint8_t* __restrict__ x, double* __restrict__ y,
                                                                 int64_t H, int64_t W, TapsIdeal2<R, C> taps,
                                                                 int rows) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ d2 sbuf[kBlock * 2];
    const int lane = threadIdx.x & (kWave - 1);
    // this wave's 256 columns
    const int64_t cw = ((int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6)) * (4 * kWave);
    if (cw >= W) return;  // wave-uniform (no block barrier below)
    x += (int64_t)blockIdx.z * H * W;  // frame blockIdx.z of a batch stored back to back
    y += (int64_t)blockIdx.z * H * W;
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    const int T = (int)(min(r0 + (int64_t)rows, H) - r0) + R - 1;  // input rows of the strip
    d2* wb = sbuf + (threadIdx.x - lane) * 2;
    if (cw + 4 * kWave <= W)
        ideal2d_strip<R, C, true>(x, y, H, W, taps, cw, lane, r0, T, wb);
    else
        ideal2d_strip<R, C, false>(x, y, H, W, taps, cw, lane, r0, T, wb);
}

// Any R x C (taps in device memory, row-major), any width, any alignment: one output per thread,
// rows grid-strided; the m / n ranges are cut to the in-frame terms (skipping a zero term is
// identical to adding it, see the header).
__global__ __launch_bounds__(kBlock) void fir2d_ideal_generic_kernel(const uint8_t* __restrict__ x,
                                                                     double* __restrict__ y, int64_t H, int64_t W,
                                                                     const double* __restrict__ taps, int R, int C) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= W) return;
    x += (int64_t)blockIdx.z * H * W;
    y += (int64_t)blockIdx.z * H * W;
    const int64_t cr = R / 2, cc = C / 2;
    // in-frame columns: 0 <= j - n + cc < W
    const int64_t n_lo = max((int64_t)0, j + cc - (W - 1)), n_hi = min((int64_t)C - 1, j + cc);
    for (int64_t i = blockIdx.y; i < H; i += gridDim.y) {
        const int64_t m_lo = max((int64_t)0, i + cr - (H - 1)), m_hi = min((int64_t)R - 1, i + cr);
        double acc = 0.0;
        for (int64_t m = m_lo; m <= m_hi; ++m) {
            const uint8_t* xr = x + (i - m + cr) * W + j + cc;
            const double* hr = taps + m * C;
            for (int64_t n = n_lo; n <= n_hi; ++n) acc = __dadd_rn(acc, __dmul_rn(hr[n], (double)xr[-n]));
        }
        y[i * W + j] = acc;
    }
}

template <int R, int C>
static hipError_t launch_ideal2d_reg(const uint8_t* x, double* y, int64_t frames, int64_t H, int64_t W,
                                     const double* h, hipStream_t s) {
    TapsIdeal2<R, C> t;
    for (int m = 0; m < R; ++m)
        for (int n = 0; n < C; ++n) t.h[m][n] = h[m * C + n];
    const int64_t rows = std::max<int64_t>(kIdeal2dStrip, (H + 65534) / 65535);  // at most 65535 strips
    const int64_t gx = (W + 4 * kBlock - 1) / (4 * kBlock), gy = (H + rows - 1) / rows;
    FIR_LAUNCH((fir2d_ideal_reg_kernel<R, C>), dim3((unsigned)gx, (unsigned)gy, (unsigned)frames), dim3(kBlock),
                       0, s, x, y, H, W, t, (int)rows);
    return hipGetLastError();
}

int check_fir2d_ideal(int64_t frames, int64_t H, int64_t W, const double* h, int R, int C, std::string* err) {
    if (H < 0 || W < 0 || frames < 0) return *err = "frames, height and width must be >= 0", FIR_EINVAL;
    if (frames > 65535) return *err = "frames must be <= 65535 per call", FIR_EINVAL;
    if (!h) return *err = "h must not be NULL", FIR_EINVAL;
    if (R < 1 || C < 1 || (int64_t)R * C > FIR_MAX_TAPS)
        return *err = "tap_rows*tap_cols must be in [1, " + std::to_string(FIR_MAX_TAPS) + "]", FIR_EINVAL;
    return FIR_OK;
}

int launch_fir2d_ideal(const uint8_t* x, int64_t frames, int64_t H, int64_t W, const double* h, int R, int C,
                       double* y, hipStream_t stream, std::string* err) {
    if (const int rc = check_fir2d_ideal(frames, H, W, h, R, C, err)) return rc;
    if (H == 0 || W == 0 || frames == 0) return FIR_OK;
    if (!x || !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    // register kernel: whole dwords per row (every row then starts 4-byte aligned in x and 16-byte
    // aligned in y), and at least one dword plus the halo; the strip height grows past 65535 strips
    const bool reg = R <= kIdeal2dMaxRC && C <= kIdeal2dMaxRC && (uintptr_t)x % 4 == 0 && (uintptr_t)y % 16 == 0 &&
                     W % 4 == 0 && W >= 4 + C - 1 && (W + 4 * kBlock - 1) / (4 * kBlock) < ((int64_t)1 << 31) &&
                     (H + 65534) / 65535 < ((int64_t)1 << 30);
    hipError_t e = hipErrorInvalidValue;
    if (reg) {
        e = with_int<1, kIdeal2dMaxRC>(R, hipErrorInvalidValue, [&](auto r) {
            constexpr int TR = decltype(r)::value;
            return with_int<1, kIdeal2dMaxRC>(C, hipErrorInvalidValue, [&](auto c) {
                return launch_ideal2d_reg<TR, c>(x, y, frames, H, W, h, stream);
            });
        });
    } else {
        if ((W + kBlock - 1) / kBlock >= ((int64_t)1 << 31)) return *err = "width too large", FIR_EINVAL;
        const double* td = (const double*)device_table(h, sizeof(double) * (size_t)R * (size_t)C, err);
        if (!td) return FIR_ENOMEM;
        TableHold hold(td, stream);
        const dim3 grid((unsigned)((W + kBlock - 1) / kBlock), (unsigned)std::min<int64_t>(H, 65535), (unsigned)frames);
        FIR_LAUNCH(fir2d_ideal_generic_kernel, grid, dim3(kBlock), 0, stream, x, y, H, W, td, R, C);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return *err = std::string("ideal2d launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace fir
