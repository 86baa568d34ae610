// fir1d_decim.hip — the decimating 1-D fixed-point FIR: filter and keep every D-th output frame.
//
//   out_width = width > phase ? (width - phase + D - 1) / D : 0
//   y[r, m, c] = y_full[r, m*D + phase, c],   y_full = what fir1d_fixed_rows gives (fir1d.hip)
//
// Arithmetic as in fir1d_lds.hip: centre L/2, zero padding at each row's ends, wrap to acc_bits,
// overflow-free round-half-up by frac_bits, u8-sat or int32 stage.  Two kernels:
//
//  * fir1d_decim_kernel — the hot path (decim_path_ok).  The tile is kDecT = 512 consecutive
//    output frames of ONE row (a tile never spans two rows, so out-of-row samples are zeroed once,
//    at staging); lane u owns outputs 2u and 2u+1 of a tile.  A workgroup owns G = max(1, 16 / D)
//    consecutive tiles of its row -- the input of one tile at D = 2 is 2 KiB, too little in flight
//    per CU to cover the HBM latency (measured with one tile per workgroup: 0.42 of the HBM peak
//    at D = 2, 0.63 at D = 8, profiles/decim) -- so every workgroup stages up to 16 * kDecT frames
//    whatever D is: the G*kDecT*D + LP - 1 input frames behind its outputs (whole 8-frame chunks,
//    all of a thread's loads issued before its first LDS write: one 16-byte load of int16, 8
//    bytes of u8 widened by v_perm, two 16-byte loads of complex int16 split into an I and a Q
//    plane set) as int16 pairs in LDS, then every lane runs LP/2 v_dot2_i32_i16 per output and
//    channel (wrap-around, no clamp) over taps passed by value: no device table, nothing
//    allocated, so the call can be captured in a graph.
//
//    LDS layout.  A lane pair of outputs is 2*D frames = D dwords apart, so a linear window
//    would put the lanes of a wave D dwords apart: an 8-way bank conflict at D = 16, 4-way at 8
//    (ds_read_b32: bank = dword mod 32 within each 32-lane half).  The staged dwords are
//    therefore stored as D polyphase planes, dword a at plane a mod D, index a / D: the window
//    dword p of output 2u+e is then at plane (q_e + p) mod D, index (q_e + p) / D + u with q_e
//    the same for every lane -- consecutive lanes read consecutive dwords of one plane, conflict
//    free for every D, and the plane / index of each p are wave-uniform (scalar) values.  Tile g
//    of the workgroup is kDecT*D frames = 256 whole plane rows further on: index + 256 g.
//
//    Pair alignment.  An output's window starts at frame m*D + phase + L/2 - (L-1) of its row.
//    The taps are reversed, padded to the even bucket LP and shifted by pf in {0, 1} zero taps
//    so that the first window of every tile starts on an even frame; the workgroup's LDS origin
//    is that frame rounded down to a multiple of 8 (a 16-byte boundary of the row).  For even D
//    every window then starts on a dword; for odd D the lane's second output (e = 1) starts on
//    an odd frame and takes its pairs through one v_alignbit each (template ODD).
//
//    LDS per workgroup: channels * (G*kDecT*D + LP + 15) * 2 bytes rounded to whole planes, with
//    G*D <= 16 at most 33.4 KiB (complex int16, LP = 130): four workgroups per CU at every D.
//    Stores: lane u writes its two consecutive output frames (2, 4, 8 or 16 bytes) in one store
//    of element alignment, so a wave writes one contiguous run at any row offset.
//
//  * fir1d_decim_generic_kernel — every other legal call (any D >= 1, any L up to FIR_MAX_TAPS,
//    any channel count or alignment, acc_bits of any width): one output per thread, taps from a
//    cached device table, exact 64-bit sums (128-bit when needs_wide says so).
#include <string>
#include <type_traits>

#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_launch.h"

namespace fir {

constexpr int kDecT = 512;        // output frames per tile: 2 per lane
constexpr int kDecMaxD = 16;      // ... and G * D <= kDecMaxD: tiles per workgroup G = max(1, 16 / D)
constexpr int kDecMaxTaps = 128;
constexpr int kDecMaxLP = 130;    // the largest tap bucket (kDecMaxTaps + pf, even)
constexpr int kDecChunk = 8;      // frames per staging step of one thread
// a / D == (a * (2^18 / D + 1)) >> 18 for a < 2^14 and 2 <= D <= 16, the product staying below 2^31 + 2^14
constexpr int kDecMagicShift = 18;

// frames a workgroup of G tiles stages: lead + the last window's start + LP + the odd form's
// extra dword, in whole chunks
__host__ __device__ constexpr int dec_chunks(int lead, int G, int D, int LP) {
    return (lead + (G * kDecT - 1) * D + LP + 2 + kDecChunk - 1) / kDecChunk;
}
constexpr int kDecMaxIt = (dec_chunks(6, kDecMaxD, 1, kDecMaxLP) + kBlock - 1) / kBlock;  // staging steps per thread
static_assert(kDecMaxIt == 5 && dec_chunks(6, 1, kDecMaxD, kDecMaxLP) <= kDecMaxIt * kBlock, "staging steps");
static_assert(4 * dec_chunks(6, kDecMaxD, 1, kDecMaxLP) < (1 << 14), "the magic division's range");

typedef uint32_t dec_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t dec_u2 __attribute__((ext_vector_type(2)));
// stores at element alignment: an output row starts at any element offset
typedef uint32_t dec_u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t dec_u2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t dec_u32_a1 __attribute__((aligned(1)));
typedef uint16_t dec_u16_a1 __attribute__((aligned(1)));

template <int LP>
struct TapsDec {
    uint32_t pk[LP / 2];  // pair p = (g[2p], g[2p+1]), g[pf + t] = h[L-1-t]: window order
};

template <typename InT, int STAGE, int CH, int LP, bool ODD>
__global__ __launch_bounds__(kBlock) void fir1d_decim_kernel(const InT* __restrict__ x,
                                                             typename OutTraits<STAGE>::T* __restrict__ y,
                                                             int64_t width, int64_t out_width, uint32_t groups, int G,
                                                             int D, int base, int PL, uint32_t magic,
                                                             TapsDec<LP> taps, int shl, int frac) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dec_lds[];  // CH plane sets of D * PL dwords
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t m0 = (int64_t)tb * G * kDecT;    // first output frame of the workgroup
    const int64_t left = (out_width - m0 + kDecT - 1) / kDecT;
    const int gt = left < G ? (int)left : G;       // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = m0 * D + base;              // its first window's first frame in the row (even, may be < 0)
    const int64_t o = a0 & ~(int64_t)(kDecChunk - 1);  // LDS origin: floor to 8 frames
    const int lead = (int)(a0 - o);                // even, 0..6
    const int nchunks = dec_chunks(lead, gt, D, LP);
    const InT* __restrict__ xr = x + r * width * CH;
    const int planes = D * PL;

    // ---- stage frames [o, o + 8 * nchunks) of the row (zero outside [0, width)): first every load
    // of the thread, as the raw dwords of memory, then the widening / channel split and the LDS writes
    constexpr int NR = kDecChunk * CH * (int)sizeof(InT) / 4;  // raw dwords per chunk
    constexpr int EP = 4 / (int)sizeof(InT);                   // samples per raw dword
    uint32_t raw[kDecMaxIt][NR];
#pragma unroll
    for (int it = 0; it < kDecMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kDecChunk;
        if (f >= 0 && f + kDecChunk <= width) {
            if constexpr (NR == 2) {
                const dec_u2 q = *reinterpret_cast<const dec_u2*>(xr + f);
                raw[it][0] = q.x;
                raw[it][1] = q.y;
            } else {
#pragma unroll
                for (int j = 0; j < NR / 4; ++j) {
                    const dec_u4 q = reinterpret_cast<const dec_u4*>(xr + f * CH)[j];
                    raw[it][4 * j] = q.x;
                    raw[it][4 * j + 1] = q.y;
                    raw[it][4 * j + 2] = q.z;
                    raw[it][4 * j + 3] = q.w;
                }
            }
        } else {  // a chunk that crosses a row end, or lies outside the row
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < EP; ++t) {
                    const int e = j * EP + t;  // sample e of the chunk: frame f + e / CH, channel e % CH
                    const int64_t fe = f + e / CH;
                    const uint32_t s = fe >= 0 && fe < width ? (uint32_t)(int32_t)xr[f * CH + e] : 0u;
                    v |= (s & (sizeof(InT) == 1 ? 0xFFu : 0xFFFFu)) << (8 * (int)sizeof(InT) * t);
                }
                raw[it][j] = v;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < kDecMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t wv[CH];  // dword i of the chunk, per channel: frames 2i and 2i + 1 as int16
            if constexpr (sizeof(InT) == 1) {
                wv[0] = __builtin_amdgcn_perm(0u, raw[it][i / 2], (i & 1) ? 0x0C030C02u : 0x0C010C00u);
            } else if constexpr (CH == 1) {
                wv[0] = raw[it][i];
            } else {  // (I, Q) dwords -> an (I, I) and a (Q, Q) dword
                wv[0] = __builtin_amdgcn_perm(raw[it][2 * i + 1], raw[it][2 * i], 0x05040100u);
                wv[1] = __builtin_amdgcn_perm(raw[it][2 * i + 1], raw[it][2 * i], 0x07060302u);
            }
            const uint32_t a = 4u * (uint32_t)k + i;
            // every factor is below 2^24: v_mul_u32_u24 (full rate) instead of v_mul_lo_u32
            const uint32_t idx = (uint32_t)__umul24(a, magic) >> kDecMagicShift;  // a / D
            const uint32_t pl = a - (uint32_t)__umul24(idx, (uint32_t)D);         // a % D
#pragma unroll
            for (int c = 0; c < CH; ++c) dec_lds[c * planes + (uint32_t)__umul24(pl, (uint32_t)PL) + idx] = wv[c];
        }
    }
    __syncthreads();

    // ---- lane u: outputs 2u and 2u + 1 of each tile g; tile g's windows are 256 g plane rows on
    const int u = threadIdx.x;
    for (int g = 0; g < gt; ++g) {
        int32_t q[2][CH];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const bool shift = ODD && e == 1;          // the window starts on an odd frame: one dword more
            const int nd = LP / 2 + (shift ? 1 : 0);
            const uint32_t s = (uint32_t)(lead + e * D);  // the window's first frame in LDS, lane 0 of tile 0
            const uint32_t q0 = s >> 1;
            const uint32_t idx0 = (q0 * magic) >> kDecMagicShift;
            const uint32_t pl0 = q0 - idx0 * (uint32_t)D;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                uint32_t d[LP / 2 + 1];
                uint32_t pl = pl0, idx = idx0 + g * (kDecT / 2);  // wave-uniform
#pragma unroll
                for (int p = 0; p < LP / 2 + 1; ++p) {
                    if (p < nd) d[p] = dec_lds[c * planes + pl * PL + idx + u];
                    if (++pl == (uint32_t)D) {
                        pl = 0;
                        ++idx;
                    }
                }
                uint32_t acc = 0;
#pragma unroll
                for (int p = 0; p < LP / 2; ++p) {
                    const uint32_t pr = shift ? __builtin_amdgcn_alignbit(d[p + 1], d[p], 16) : d[p];
                    acc = dot2_acc(pr, taps.pk[p], acc);
                }
                q[e][c] = round32(acc, shl, frac);
            }
        }

        const int64_t m = m0 + (int64_t)g * kDecT + 2 * u;
        if (m >= out_width) break;  // only in the row's last tile
        const bool two = m + 1 < out_width;
        typename OutTraits<STAGE>::T* yo = y + (r * out_width + m) * CH;
        if constexpr (STAGE == FIR_OUT_I32) {
            if constexpr (CH == 1) {
                if (two)
                    *reinterpret_cast<dec_u2_a4*>(yo) = dec_u2_a4{(uint32_t)q[0][0], (uint32_t)q[1][0]};
                else
                    yo[0] = q[0][0];
            } else {
                if (two)
                    *reinterpret_cast<dec_u4_a4*>(yo) =
                        dec_u4_a4{(uint32_t)q[0][0], (uint32_t)q[0][1], (uint32_t)q[1][0], (uint32_t)q[1][1]};
                else
                    *reinterpret_cast<dec_u2_a4*>(yo) = dec_u2_a4{(uint32_t)q[0][0], (uint32_t)q[0][1]};
            }
        } else {
            if constexpr (CH == 1) {
                const uint32_t b0 = stage_out32<STAGE>(q[0][0]), b1 = stage_out32<STAGE>(q[1][0]);
                if (two)
                    *reinterpret_cast<dec_u16_a1*>(yo) = (uint16_t)(b0 | (b1 << 8));
                else
                    yo[0] = (uint8_t)b0;
            } else {
                const uint32_t b0 = stage_out32<STAGE>(q[0][0]), b1 = stage_out32<STAGE>(q[0][1]);
                const uint32_t b2 = stage_out32<STAGE>(q[1][0]), b3 = stage_out32<STAGE>(q[1][1]);
                if (two)
                    *reinterpret_cast<dec_u32_a1*>(yo) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                else
                    *reinterpret_cast<dec_u16_a1*>(yo) = (uint16_t)(b0 | (b1 << 8));
            }
        }
    }
}

// One output per thread: output gi = ((r * out_width + m) * ch + c) sums the taps whose sample
// lies in row r (the in-row test of fir1d_generic_kernel, as loop bounds).
template <typename InT, int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_decim_generic_kernel(const InT* __restrict__ x,
                                                                     typename OutTraits<STAGE>::T* __restrict__ y,
                                                                     int64_t n_out, int64_t width, int64_t out_width,
                                                                     int64_t ch, int64_t D, int64_t phase,
                                                                     const int32_t* __restrict__ taps, int L, int frac,
                                                                     int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t c = gi % ch, t = gi / ch;
    const int64_t m = t % out_width, r = t / out_width;
    const int64_t n = m * D + phase + L / 2;  // tap k reads frame n - k
    // 0 <= n - k < width  <=>  n - width < k <= n
    const int64_t k_lo = n - width + 1 > 0 ? n - width + 1 : 0;
    const int64_t k_hi = n < L - 1 ? n : L - 1;
    const InT* __restrict__ xr = x + r * width * ch + c;
    using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
    using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;
    Acc acc = 0;
    for (int64_t k = k_lo; k <= k_hi; ++k) acc += (Acc)(SAcc)((int64_t)taps[k] * (int32_t)xr[(n - k) * ch]);
    if constexpr (WIDE)
        y[gi] = stage_out128<STAGE>(round128((__int128)acc, frac, acc_bits));
    else
        y[gi] = stage_out<STAGE>(round64((int64_t)acc, frac, acc_bits));
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t decim_out_width(int64_t width, int decim, int phase) {
    if (width < 0 || decim < 1 || phase < 0 || phase >= decim) return -1;
    return width > phase ? (width - phase - 1) / decim + 1 : 0;  // ceil without overflow near 2^63
}

int check_fir1d_decim(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int decim,
                      int phase, int frac, int acc_bits, int stage, int64_t* out_width, std::string* err) {
    const int rc = check_fir1d(in_dtype, rows, width, ch, hq, L, 1, frac, acc_bits, stage, err);
    if (rc) return rc;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    int64_t rw = 0, n = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || __builtin_mul_overflow(rw, (int64_t)ch, &n) || n > INT64_MAX / 4)
        return *err = "invalid rows/width/channels", FIR_EINVAL;
    *out_width = decim_out_width(width, decim, phase);
    return FIR_OK;
}

bool decim_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                   int decim, int frac, int acc_bits, int64_t out_width) {
    if (decim < 2 || decim > kDecMaxD || L > kDecMaxTaps || acc_bits > 32 || frac > 31) return false;
    if (!(ch == 1 || (ch == 2 && in_dtype == FIR_IN_I16))) return false;
    for (int k = 0; k < L; ++k)
        if (hq[k] < -32768 || hq[k] > 32767) return false;
    const int64_t rowlen = width * ch;
    if ((uintptr_t)x % (in_dtype == FIR_IN_U8 ? 8 : 16) != 0) return false;
    if (!(rows == 1 || rowlen % 8 == 0)) return false;  // every row starts as x does
    const int64_t tiles = (out_width + kDecT - 1) / kDecT;
    // the grid is rows * tiles workgroups; the kernel holds a tile index in 32 bits
    return width < ((int64_t)1 << 40) && tiles < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31) / tiles;
}

template <typename InT, int STAGE, int CH, int LP, bool ODD>
static hipError_t launch_decim_lp(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width,
                                  const int32_t* hq, int L, int D, int phase, int pf, int frac, int acc_bits,
                                  hipStream_t s) {
    int32_t g[LP] = {};
    for (int t = 0; t < L; ++t) g[pf + t] = hq[L - 1 - t];
    TapsDec<LP> taps;
    for (int p = 0; p < LP / 2; ++p) taps.pk[p] = ((uint32_t)g[2 * p] & 0xFFFFu) | ((uint32_t)g[2 * p + 1] << 16);
    const int base = phase + L / 2 - (L - 1) - pf;  // even
    const int G = D >= kDecMaxD ? 1 : kDecMaxD / D;  // tiles per workgroup: G * D <= 16
    const int PL = (dec_chunks(6, G, D, LP) * 4 + D - 1) / D;  // dwords per plane (lead <= 6)
    const uint32_t magic = (1u << kDecMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (out_width + (int64_t)G * kDecT - 1) / ((int64_t)G * kDecT);
    const size_t lds = (size_t)CH * D * PL * sizeof(uint32_t);
    using OutT = typename OutTraits<STAGE>::T;
    FIR_LAUNCH((fir1d_decim_kernel<InT, STAGE, CH, LP, ODD>), dim3((unsigned)(rows * groups)), dim3(kBlock),
                       lds, s, (const InT*)x, (OutT*)y, width, out_width, (uint32_t)groups, G, D, base, PL, magic,
                       taps, 32 - acc_bits, frac);
    return hipGetLastError();
}

template <typename InT, int STAGE, int CH>
static hipError_t launch_decim_ch(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width,
                                  const int32_t* hq, int L, int D, int phase, int frac, int acc_bits, hipStream_t s) {
    // pf zero taps in front make every tile's first window start on an even frame of its row
    const int pf = (phase + L / 2 - (L - 1)) & 1;
    const int need = L + pf;
    const auto go = [&](auto lp) {
        constexpr int LP = decltype(lp)::value;
        if (D & 1)
            return launch_decim_lp<InT, STAGE, CH, LP, true>(x, y, rows, width, out_width, hq, L, D, phase, pf, frac,
                                                             acc_bits, s);
        return launch_decim_lp<InT, STAGE, CH, LP, false>(x, y, rows, width, out_width, hq, L, D, phase, pf, frac,
                                                          acc_bits, s);
    };
    if (need <= 8) return go(IntTag<8>{});
    if (need <= 16) return go(IntTag<16>{});
    if (need <= 24) return go(IntTag<24>{});
    if (need <= 32) return go(IntTag<32>{});
    if (need <= 48) return go(IntTag<48>{});
    if (need <= 64) return go(IntTag<64>{});
    if (need <= 96) return go(IntTag<96>{});
    return go(IntTag<130>{});  // kDecMaxTaps + pf
}

template <typename InT, int STAGE>
static hipError_t launch_decim_generic(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width, int ch,
                                       const int32_t* hq, int L, int D, int phase, int frac, int acc_bits,
                                       hipStream_t s) {
    using OutT = typename OutTraits<STAGE>::T;
    const int64_t n_out = rows * out_width * ch;
    const int64_t blocks = (n_out + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    std::string err;
    const int32_t* td = (const int32_t*)device_table(hq, sizeof(int32_t) * (size_t)L, &err);
    if (!td) return hipErrorOutOfMemory;
    TableHold hold(td, s);
    if (needs_wide(sizeof(InT) == 1 ? FIR_IN_U8 : FIR_IN_I16, hq, L, acc_bits))
        FIR_LAUNCH((fir1d_decim_generic_kernel<InT, STAGE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, out_width, (int64_t)ch, (int64_t)D, (int64_t)phase,
                           td, L, frac, acc_bits);
    else
        FIR_LAUNCH((fir1d_decim_generic_kernel<InT, STAGE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, out_width, (int64_t)ch, (int64_t)D, (int64_t)phase,
                           td, L, frac, acc_bits);
    return hipGetLastError();
}

int launch_fir1d_decim(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                       int decim, int phase, int frac, int acc_bits, int stage, void* y, hipStream_t stream,
                       std::string* err) {
    int64_t ow = 0;
    const int rc = check_fir1d_decim(in_dtype, rows, width, ch, hq, L, decim, phase, frac, acc_bits, stage, &ow, err);
    if (rc) return rc;
    if (rows == 0 || ow == 0) return FIR_OK;
    if (!x || !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    const bool fast = decim_path_ok(x, in_dtype, rows, width, ch, hq, L, decim, frac, acc_bits, ow);
    const hipError_t e = with_io(in_dtype, stage, [&](auto t, auto st) {
        using InT = typename decltype(t)::type;
        if (!fast)
            return launch_decim_generic<InT, st>(x, y, rows, width, ow, ch, hq, L, decim, phase, frac, acc_bits, stream);
        if constexpr (sizeof(InT) == 2) {
            if (ch == 2)
                return launch_decim_ch<InT, st, 2>(x, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits, stream);
        }
        return launch_decim_ch<InT, st, 1>(x, y, rows, width, ow, hq, L, decim, phase, frac, acc_bits, stream);
    });
    if (e != hipSuccess) return *err = std::string("fir1d decim launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace fir
