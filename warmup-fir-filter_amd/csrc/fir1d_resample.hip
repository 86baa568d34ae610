// fir1d_resample.hip — the rational U/D resampling 1-D fixed-point FIR: zero-stuff by U, filter,
// keep every D-th output frame, in one pass.
//
//   mid_width  = width * U
//   out_width  = mid_width > phase ? (mid_width - phase + D - 1) / D : 0
//   y[r, m, c] = y_up[r, m*D + phase, c],   y_up = what fir_interp_rows gives (fir1d_interp.hip)
//
// so the same centre rule (L/2), zero padding at each row's ends, wrap to acc_bits, round-half-up
// by frac_bits, u8-sat or int32 stage, and no gain.  U = 1 is the decimator and D = 1 the
// interpolator: launch_fir1d_resample forwards both to their own (tuned) launchers.
//
// Polyphase form.  With a_q = phase + L/2 + q*D, p_q = a_q mod U, c_q = a_q div U, output
// m = v*U + q (0 <= q < U) of a row is
//
//   acc = sum over t >= 0, p_q + U*t < L of hq[p_q + U*t] * x[r, v*D + c_q - t, c]
//
// p_q and c_q depend on q alone and the pattern repeats every U outputs = D input frames (one
// PERIOD v): no stuffed zero is multiplied, no dropped output is computed.  Two kernels:
//
//  * fir1d_resample_kernel — the hot path (resample_path_ok).  A workgroup owns P consecutive
//    periods of ONE row (never two rows, so out-of-row frames are zeroed once, at staging): P =
//    256 doubled until P * D * in_size >= 4096 bytes, i.e. at least 4 KiB (less than 8 KiB) of input
//    per channel in flight per workgroup (int16: P = 1024 at D = 2 or 3, 512 up to D = 7, 256 from
//    D = 8 on; u8: twice that).  It works through them as G = P / T tiles of T periods, T = P
//    halved while the tile's outputs T * U * channels * out_size exceed 16 KiB, but not below 256.
//    A tile is computed in passes of 512 periods: lane u owns periods 2u and 2u + 1 of every pass
//    and produces their 2U consecutive output frames (a tile of 256 periods is half a pass: two
//    waves compute).  One pass is B = 512 U output frames, one tile T U, one workgroup P U.
//
//    Input, as in the decimator.  The workgroup stages the frames behind all of its outputs (whole
//    8-frame chunks, all of a thread's loads issued before its first LDS write: 16 bytes of int16,
//    8 bytes of u8 widened by v_perm, two 16-byte loads of complex int16 split into an I and a Q
//    plane set) as int16 pairs.  A lane's pair of periods is 2D frames = D dwords from the next
//    lane's, so the dwords are stored as D polyphase planes, dword a at plane a mod D, index a / D:
//    consecutive lanes read consecutive dwords of one plane for every D, conflict free, and the
//    plane / index of every read are wave-uniform values plus the lane.  LDS dword 0 is the first
//    window's first frame, S = the lowest c_q - n_q + 1 floored to even (n_q = taps of phase q);
//    the loads start at that frame rounded down to 8.  Per q the sub-filter is in window order with
//    one leading zero tap where its window would start on an odd frame, zero padded to the bucket
//    NP, as int16 pairs passed BY VALUE next to the window's first dword k0_q and a table of the
//    LDS offset (k mod D) * PL + k / D of every window dword k, two 16-bit offsets per entry (at
//    most 16 * 34 + 16 + 64 dwords of kernarg, read with scalar loads of consecutive entries): no
//    device table, nothing allocated, so the call can be captured in a graph.  The table is what
//    the measurement asked for: stepping plane and index per read as the decimator does costs five
//    scalar instructions a read, and with a read per v_dot2 those bounded the kernel at twice the
//    time (profiles/resample).  The second period's window lies D frames on: for odd D it starts
//    on an odd frame and takes its pairs through one v_alignbit each.  Arithmetic: NP
//    v_dot2_i32_i16 per output and channel (wrap-around, no clamp), round32, stage_out32; a bucket
//    past 18 pairs runs as two halves per phase, so that the taps and offsets of one body fit the
//    SGPRs.
//
//    Output, as in the interpolator.  Every result goes to an LDS output stage at the byte it has
//    in the tile's output run (byte b at b + 4 * (b / 128): one pad dword per 32), which starts
//    (y address mod 16) bytes in, so that LDS vectors and global vectors line up for ANY y address;
//    the run is then written as whole 16-byte vectors, consecutive lanes consecutive vectors, the
//    partial vector at either end element by element, inside the tile's own bytes.  The row's last
//    period is masked at m < out_width: the run ends there.
//
//    LDS per workgroup: channels * (P * D + about D + 2 NP + 16) * 2 bytes of input in whole planes
//    (under 16.5 KiB: u8 or complex int16 at D = 15) plus T * U * channels * out_size + 16 bytes of
//    stage with its padding (16.5 KiB; 33 KiB where T = 256 is the floor, complex int32 at U = 16):
//    under 50 KiB at every (U, D, type), so at least three workgroups per CU of 160 KiB.
//
//  * fir1d_resample_generic_kernel — every other legal call (any U, D >= 1, any L up to
//    FIR_MAX_TAPS, any channel count or alignment, acc_bits of any width): one output per thread,
//    the interpolator's generic kernel at j = m * D + phase, taps from a cached device table,
//    exact 64-bit sums (128-bit when needs_wide says so).
#include <string>
#include <type_traits>

#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_launch.h"

namespace fir {

constexpr int kResInBytes = 4096;     // input bytes per channel a workgroup keeps in flight, at least
constexpr int kResPass = 512;         // periods per pass of the workgroup: 2 per lane
constexpr int kResMinT = 256;         // the smallest tile and workgroup: half a pass, two waves compute
constexpr int kResOutBytes = 16384;   // T = P halved while T * U * channels * out_size exceeds this
constexpr int kResMaxUD = 16;         // 2 <= U, D <= 16
constexpr int kResMaxPhaseTaps = 64;  // ceil(L / U) <= 64
constexpr int kResMaxNP = 33;         // the largest pair bucket: 64 taps + the leading zero
constexpr int kResChunk = 8;          // frames per staging step of one thread
constexpr int kResOffs = 64;          // window dwords a lane can address (the highest k0 + D / 2 + NQ + 1 is 52)
// a / D == (a * (2^18 / D + 1)) >> 18 for a < 2^14 and 2 <= D <= 16 (as the decimator's)
constexpr int kResMagicShift = 18;

// periods per workgroup
__host__ __device__ constexpr int res_periods(int in_size, int D) {
    int P = kResMinT;
    while (P * D * in_size < kResInBytes) P *= 2;
    return P;
}
// chunks a workgroup of n periods stages: lead + the last period's first frame + ext, the frames
// from there to the end of the furthest window (the highest window offset + 2 NQ + 2)
__host__ __device__ constexpr int res_chunks(int lead, int n, int D, int ext) {
    return (lead + (n - 1) * D + ext + kResChunk - 1) / kResChunk;
}
// the largest ext: window offsets up to D + 2 frames, the largest bucket
constexpr int kResMaxExt = kResMaxUD + 2 + 2 * (kResMaxNP + 1) + 2;
// staging steps per thread: 5 of u8, 3 of int16; P * D * in_size < 2 * kResInBytes
__host__ __device__ constexpr int res_steps(int in_size) {
    return (res_chunks(6, kResInBytes / in_size, 2, kResMaxExt) + kBlock - 1) / kBlock;
}
static_assert(res_steps(1) == 5 && res_steps(2) == 3, "staging steps");
static_assert(4 * res_steps(1) * kBlock < (1 << 14), "the magic division's range");

// the output stage: logical byte b at b + 4 * (b / 128)
__host__ __device__ constexpr uint32_t res_phys(uint32_t b) { return b + ((b >> 7) << 2); }

typedef uint32_t res_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t res_u2 __attribute__((ext_vector_type(2)));

// A bucket past 18 pairs is computed as two halves of HP pairs each (the taps, the offsets of two windows and the
// rest of one body of 33 pairs do not fit the SGPRs): NH halves, NQ = NH * HP pairs per phase in the table
__host__ __device__ constexpr int res_halves(int NP) { return NP > 18 ? 2 : 1; }
__host__ __device__ constexpr int res_hp(int NP) { return (NP + res_halves(NP) - 1) / res_halves(NP); }
__host__ __device__ constexpr int res_nq(int NP) { return res_halves(NP) * res_hp(NP); }
static_assert(res_nq(kResMaxNP) == 34 && kResMaxUD / 2 + 1 + kResMaxUD / 2 + res_nq(kResMaxNP) + 2 <= kResOffs,
              "k0 <= D / 2 + 1; the second window starts D / 2 dwords on and reads NQ + 1");

template <int NP>
struct TapsRes {
    uint32_t pk[kResMaxUD * res_nq(NP)];  // phase q, pair p at q * NQ + p: (g_q[2p], g_q[2p+1]) in window order
    uint32_t k0[kResMaxUD];       // phase q: its window's first dword, from the lane's first window dword
    // window dword k of a lane lies (k mod D) * PL + k / D dwords from the lane's own plane row: entry
    // par * kResOffs / 2 + i holds that offset for k = par + 2 i in its low half and for k + 1 in its
    // high half, so a window from any k reads consecutive entries of the table of its parity
    uint32_t off[kResOffs];
};

template <typename InT, int STAGE, int CH, int NP>
__global__ __launch_bounds__(kBlock) void fir1d_resample_kernel(const InT* __restrict__ x,
                                                                typename OutTraits<STAGE>::T* __restrict__ y,
                                                                int64_t width, int64_t out_width, uint32_t groups, int U,
                                                                int D, int P, int T, int S, int ext, int PL,
                                                                uint32_t magic, TapsRes<NP> taps, int shl, int frac) {
    using OutT = typename OutTraits<STAGE>::T;
    constexpr int OS = (int)sizeof(OutT);
    constexpr int kMaxIt = res_steps((int)sizeof(InT));
    constexpr int NH = res_halves(NP), HP = res_hp(NP), NQ = res_nq(NP);
    extern __shared__ __attribute__((aligned(16))) uint32_t res_lds[];  // CH plane sets of D * PL dwords, then the stage
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t v0 = (int64_t)tb * P;     // first period of the workgroup (even)
    const int64_t m0 = v0 * U;              // ... and its first output frame
    const int TU = T * U;                   // output frames per tile
    const int64_t left = (out_width - m0 + TU - 1) / TU;
    const int gt = left < P / T ? (int)left : P / T;   // its tiles (the row's last workgroup: fewer)
    const int64_t a0 = v0 * D + S;                     // its first window's first frame (even, may be < 0)
    const int64_t o = a0 & ~(int64_t)(kResChunk - 1);  // the first frame staged: floor to 8 frames
    const int lead = (int)(a0 - o);                    // even, 0..6
    const int nchunks = res_chunks(lead, gt * T, D, ext);
    const InT* __restrict__ xr = x + r * width * CH;
    const int planes = D * PL;

    // ---- stage frames [o, o + 8 * nchunks) of the row (zero outside [0, width)): first every load
    // of the thread, as the raw dwords of memory, then the widening / channel split and the LDS writes
    constexpr int NR = kResChunk * CH * (int)sizeof(InT) / 4;  // raw dwords per chunk
    constexpr int EP = 4 / (int)sizeof(InT);                   // samples per raw dword
    uint32_t raw[kMaxIt][NR];
#pragma unroll
    for (int it = 0; it < kMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kResChunk;
        if (f >= 0 && f + kResChunk <= width) {
            if constexpr (NR == 2) {
                const res_u2 q = *reinterpret_cast<const res_u2*>(xr + f);
                raw[it][0] = q.x;
                raw[it][1] = q.y;
            } else {
#pragma unroll
                for (int j = 0; j < NR / 4; ++j) {
                    const res_u4 q = reinterpret_cast<const res_u4*>(xr + f * CH)[j];
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
    for (int it = 0; it < kMaxIt; ++it) {
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
            const int ai = 4 * k + i - (lead >> 1);  // LDS dword 0 is the first window's first dword (frame a0)
            if (ai < 0) continue;                    // the up to 3 dwords in front of it are never read
            const uint32_t a = (uint32_t)ai;
            // every factor is below 2^24: v_mul_u32_u24 (full rate) instead of v_mul_lo_u32
            const uint32_t idx = (uint32_t)__umul24(a, magic) >> kResMagicShift;  // a / D
            const uint32_t pl = a - (uint32_t)__umul24(idx, (uint32_t)D);         // a % D
#pragma unroll
            for (int c = 0; c < CH; ++c) res_lds[c * planes + (uint32_t)__umul24(pl, (uint32_t)PL) + idx] = wv[c];
        }
    }
    __syncthreads();

    uint32_t* const outw = res_lds + CH * planes;
    uint8_t* const outb = reinterpret_cast<uint8_t*>(outw);
    const int u = threadIdx.x;
    const uint32_t odd = (uint32_t)(D & 1) << 4;  // the second period's windows start on an odd frame
    for (int g = 0; g < gt; ++g) {
        const int64_t mg = m0 + (int64_t)g * TU;  // the tile's first output frame
        const int no = out_width - mg < TU ? (int)(out_width - mg) : TU;  // its output frames inside the row
        char* const yt = reinterpret_cast<char*>(y + (r * out_width + mg) * CH);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(yt) & 15u);  // the stage's first byte

        // ---- lane u: the 2U outputs of periods 2u and 2u + 1 of every pass (kResPass periods of the
        // tile; a tile of kResMinT periods is half a pass), into the stage
        const uint32_t qstep = (uint32_t)(CH * OS);      // bytes from output q to q + 1
        const uint32_t vstep = (uint32_t)U * qstep;      // ... from a period to the next
        for (int vp = 2 * u; vp < T && vp * U < no; vp += kResPass) {  // vp: the lane's even period in the tile
            const uint32_t w = (uint32_t)(g * T + vp) >> 1;  // its plane row: dword w * D is its first window dword
#pragma unroll 1  // one channel at a time: with both in one body their scalar addresses and taps spill SGPRs
            for (int c = 0; c < CH; ++c) {
                uint32_t b = sh + (uint32_t)vp * vstep + (uint32_t)(c * OS);  // period vp, output 0, channel c
                const uint32_t cb = (uint32_t)(c * planes);  // the channel's plane set
                uint32_t acc0 = 0, acc1 = 0;
                for (int it = 0; it < U * NH; ++it) {  // phase q, half h of its pairs
                    const int q = NH == 1 ? it : it >> 1, h = NH == 1 ? 0 : it & 1;
                    const uint32_t* __restrict__ tp = taps.pk + q * NQ + h * HP;  // wave-uniform
                    // the windows' LDS offsets come from the table, consecutive entries by scalar loads: walking
                    // plane and index per read costs five scalar instructions each, which bound the kernel
                    const uint32_t ka = taps.k0[q] + (uint32_t)(h * HP);  // period vp
                    const uint32_t kb = ka + (uint32_t)(D >> 1);          // period vp + 1: D frames on
                    const uint32_t* __restrict__ oa = taps.off + (ka & 1u) * (kResOffs / 2) + (ka >> 1);
                    const uint32_t* __restrict__ ob = taps.off + (kb & 1u) * (kResOffs / 2) + (kb >> 1);
                    uint32_t d0[HP], d1[HP + 1];
#pragma unroll
                    for (int p = 0; p < HP; ++p)
                        d0[p] = res_lds[cb + w + ((p & 1) ? oa[p >> 1] >> 16 : oa[p >> 1] & 0xFFFFu)];
#pragma unroll
                    for (int p = 0; p < HP + 1; ++p)
                        d1[p] = res_lds[cb + w + ((p & 1) ? ob[p >> 1] >> 16 : ob[p >> 1] & 0xFFFFu)];
                    if (h == 0) acc0 = acc1 = 0;
#pragma unroll
                    for (int p = 0; p < HP; ++p) {
                        acc0 = dot2_acc(d0[p], tp[p], acc0);
                        acc1 = dot2_acc(__builtin_amdgcn_alignbit(d1[p + 1], d1[p], odd), tp[p], acc1);
                    }
                    if (h != NH - 1) continue;
                    const OutT q0 = stage_out32<STAGE>(round32(acc0, shl, frac));
                    const OutT q1 = stage_out32<STAGE>(round32(acc1, shl, frac));
                    if constexpr (OS == 4) {
                        outw[res_phys(b) >> 2] = (uint32_t)q0;
                        outw[res_phys(b + vstep) >> 2] = (uint32_t)q1;
                    } else {
                        outb[res_phys(b)] = q0;
                        outb[res_phys(b + vstep)] = q1;
                    }
                    b += qstep;
                }
            }
        }
        __syncthreads();

        // ---- the tile's output run [sh, end) of the stage, as 16-byte vectors at 16-byte addresses
        const uint32_t end = sh + (uint32_t)no * (uint32_t)(CH * OS);
        const uint32_t nvec = (end + 15u) >> 4;
        for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) {
            const uint32_t lo = 16u * v;
            if (lo >= sh && lo + 16u <= end) {
                res_u4 q;
                q.x = outw[res_phys(lo) >> 2];
                q.y = outw[res_phys(lo + 4) >> 2];
                q.z = outw[res_phys(lo + 8) >> 2];
                q.w = outw[res_phys(lo + 12) >> 2];
                *reinterpret_cast<res_u4*>(yt - sh + lo) = q;
            } else {  // the partial vector at either end of the run
                const uint32_t b0 = lo < sh ? sh : lo, b1 = lo + 16u < end ? lo + 16u : end;
                for (uint32_t b = b0; b < b1; b += OS) {
                    if constexpr (OS == 4)
                        *reinterpret_cast<uint32_t*>(yt - sh + b) = outw[res_phys(b) >> 2];
                    else
                        *reinterpret_cast<uint8_t*>(yt - sh + b) = outb[res_phys(b)];
                }
            }
        }
        __syncthreads();  // the next tile overwrites the stage
    }
}

// One output per thread: output gi = ((r * out_width + m) * ch + c) is frame j = m * D + phase of
// the interpolated row, j = i * U + e, and sums the taps p_e + U * t whose sample i + c_e - t lies
// in row r (the in-row test as loop bounds).
template <typename InT, int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_resample_generic_kernel(const InT* __restrict__ x,
                                                                        typename OutTraits<STAGE>::T* __restrict__ y,
                                                                        int64_t n_out, int64_t width, int64_t out_width,
                                                                        int64_t ch, int64_t U, int64_t D, int64_t phase,
                                                                        const int32_t* __restrict__ taps, int L, int frac,
                                                                        int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t c = gi % ch, q = gi / ch;
    const int64_t m = q % out_width, r = q / out_width;
    const int64_t j = m * D + phase;  // < width * U
    const int64_t i = j / U, e = j % U;
    const int64_t pe = (e + L / 2) % U, n = i + (e + L / 2) / U;  // tap pe + U * t reads frame n - t
    // 0 <= n - t < width  <=>  n - width < t <= n;  pe + U * t <= L - 1
    const int64_t t_lo = n - width + 1 > 0 ? n - width + 1 : 0;
    const int64_t t_max = pe < L ? (L - 1 - pe) / U : -1;
    const int64_t t_hi = n < t_max ? n : t_max;
    const InT* __restrict__ xr = x + r * width * ch + c;
    using Acc = typename std::conditional<WIDE, unsigned __int128, uint64_t>::type;
    using SAcc = typename std::conditional<WIDE, __int128, int64_t>::type;
    Acc acc = 0;
    for (int64_t t = t_lo; t <= t_hi; ++t) acc += (Acc)(SAcc)((int64_t)taps[pe + U * t] * (int32_t)xr[(n - t) * ch]);
    if constexpr (WIDE)
        y[gi] = stage_out128<STAGE>(round128((__int128)acc, frac, acc_bits));
    else
        y[gi] = stage_out<STAGE>(round64((int64_t)acc, frac, acc_bits));
}

// ---------------------------------------------------------------------------------------
// Host side.

int64_t resample_out_width(int64_t width, int up, int decim, int phase) {
    const int64_t mid = interp_out_width(width, up);
    return mid < 0 ? -1 : decim_out_width(mid, decim, phase);
}

int check_fir1d_resample(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up, int decim,
                         int phase, int frac, int acc_bits, int stage, int64_t* out_width, std::string* err) {
    const int rc = check_fir1d(in_dtype, rows, width, ch, hq, L, 1, frac, acc_bits, stage, err);
    if (rc) return rc;
    if (up < 1) return *err = "up must be >= 1", FIR_EINVAL;
    if (decim < 1) return *err = "decim must be >= 1", FIR_EINVAL;
    if (phase < 0 || phase >= decim) return *err = "phase must be in [0, decim)", FIR_EINVAL;
    const int64_t ow = resample_out_width(width, up, decim, phase);
    int64_t ro = 0, no = 0, rw = 0, ni = 0;
    if (ow < 0 || __builtin_mul_overflow(rows, ow, &ro) || __builtin_mul_overflow(ro, (int64_t)ch, &no) ||
        no > INT64_MAX / 4 || __builtin_mul_overflow(rows, width, &rw) || __builtin_mul_overflow(rw, (int64_t)ch, &ni) ||
        ni > INT64_MAX / 4)
        return *err = "width * up, rows * out_width * channels * 4 and rows * width * channels * 4 must fit in int64",
               FIR_EINVAL;
    *out_width = ow;
    return FIR_OK;
}

namespace {

// The U windows of a period.  Phase q: p the first tap, c the frame (from the period's first) that
// tap meets, n the taps; k0 the first dword of its window counted from S, the first frame of the
// lowest window floored to even; need: the pairs of the longest sub-filter with its leading zero.
struct ResPlan {
    int S = 0, ext = 0, need = 1;
    int p[kResMaxUD] = {}, c[kResMaxUD] = {}, n[kResMaxUD] = {}, k0[kResMaxUD] = {};
};

ResPlan res_plan(int L, int U, int D, int phase) {
    ResPlan pl;
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
    }
    pl.S = lo - (lo & 1);
    int emax = 0;
    for (int q = 0; q < U; ++q) {
        if (!pl.n[q]) continue;
        const int e = pl.c[q] - pl.n[q] + 1 - pl.S;  // >= 0; odd: one leading zero tap
        pl.k0[q] = e / 2;
        if (2 * pl.k0[q] > emax) emax = 2 * pl.k0[q];
        const int pairs = (pl.n[q] + (e & 1) + 1) / 2;
        if (pairs > pl.need) pl.need = pairs;
    }
    pl.ext = emax;  // + 2 NP + 2 once the bucket is known
    return pl;
}

// periods per tile: the workgroup's periods, halved while the tile's outputs exceed kResOutBytes
int res_tile(int P, int U, int ch, int stage) {
    int T = P;
    while (T > kResMinT && T * U * ch * (int)out_size(stage) > kResOutBytes) T /= 2;
    return T;
}

}  // namespace

bool resample_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up,
                      int decim, int frac, int acc_bits, int64_t out_width) {
    if (up < 2 || up > kResMaxUD || decim < 2 || decim > kResMaxUD || acc_bits > 32 || frac > 31) return false;
    if ((L + up - 1) / up > kResMaxPhaseTaps) return false;
    if (!(ch == 1 || (ch == 2 && in_dtype == FIR_IN_I16))) return false;
    for (int k = 0; k < L; ++k)
        if (hq[k] < -32768 || hq[k] > 32767) return false;
    const int64_t rowlen = width * ch;
    if ((uintptr_t)x % (in_dtype == FIR_IN_U8 ? 8 : 16) != 0) return false;
    if (!(rows == 1 || rowlen % 8 == 0)) return false;  // every row starts as x does
    const int64_t per = (int64_t)res_periods((int)in_size(in_dtype), decim) * up;  // output frames per workgroup
    const int64_t groups = (out_width + per - 1) / per;
    // the grid is rows * groups workgroups; the kernel holds a group index in 32 bits
    return width < ((int64_t)1 << 40) && groups < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31) / groups;
}

template <typename InT, int STAGE, int CH, int NP>
static hipError_t launch_res_np(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width,
                                const int32_t* hq, int U, int D, const ResPlan& pl, int frac, int acc_bits,
                                hipStream_t s) {
    TapsRes<NP> taps = {};
    const int P = res_periods((int)sizeof(InT), D);
    constexpr int NQ = res_nq(NP);
    const int ext = pl.ext + 2 * NQ + 2;
    const int chunks = res_chunks(6, P, D, ext);  // lead <= 6
    if (chunks > res_steps((int)sizeof(InT)) * kBlock) return hipErrorInvalidValue;  // never: kResMaxExt bounds ext
    const int PL = (chunks * 4 + D - 1) / D;      // dwords per plane
    if (pl.ext / 2 + D / 2 + NQ + 2 > kResOffs || D * PL > 0xFFFF) return hipErrorInvalidValue;  // never, as above
    const auto off = [&](int k) { return (uint32_t)((k % D) * PL + k / D); };
    for (int par = 0; par < 2; ++par)
        for (int i = 0; i < kResOffs / 2; ++i)
            taps.off[par * (kResOffs / 2) + i] = off(par + 2 * i) | (off(par + 2 * i + 1) << 16);
    for (int q = 0; q < U; ++q) {
        taps.k0[q] = (uint32_t)pl.k0[q];
        int32_t g[2 * NQ] = {};  // g[k]: the tap of frame S + 2 k0 + k of the period, i.e. t = c - S - 2 k0 - k
        for (int k = 0; k < 2 * NQ; ++k) {
            const int t = pl.c[q] - pl.S - 2 * pl.k0[q] - k;
            if (t >= 0 && t < pl.n[q]) g[k] = hq[pl.p[q] + U * t];
        }
        for (int p = 0; p < NQ; ++p)
            taps.pk[q * NQ + p] = ((uint32_t)g[2 * p] & 0xFFFFu) | ((uint32_t)g[2 * p + 1] << 16);
    }
    using OutT = typename OutTraits<STAGE>::T;
    const int T = res_tile(P, U, CH, STAGE);
    const int in_dwords = (CH * D * PL + 3) & ~3;
    const uint32_t stage_bytes = (uint32_t)(T * U * CH) * (uint32_t)sizeof(OutT) + 16u;
    const size_t lds = (size_t)in_dwords * sizeof(uint32_t) + res_phys(stage_bytes) + 4;
    const uint32_t magic = (1u << kResMagicShift) / (uint32_t)D + 1;
    const int64_t groups = (out_width + (int64_t)P * U - 1) / ((int64_t)P * U);
    FIR_LAUNCH((fir1d_resample_kernel<InT, STAGE, CH, NP>), dim3((unsigned)(rows * groups)), dim3(kBlock), lds, s,
                       (const InT*)x, (OutT*)y, width, out_width, (uint32_t)groups, U, D, P, T, pl.S, ext, PL, magic,
                       taps, 32 - acc_bits, frac);
    return hipGetLastError();
}

template <typename InT, int STAGE, int CH>
static hipError_t launch_res_ch(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width,
                                const int32_t* hq, int L, int U, int D, int phase, int frac, int acc_bits,
                                hipStream_t s) {
    const ResPlan pl = res_plan(L, U, D, phase);
    const auto go = [&](auto np) {
        return launch_res_np<InT, STAGE, CH, decltype(np)::value>(x, y, rows, width, out_width, hq, U, D, pl, frac,
                                                                  acc_bits, s);
    };
    if (pl.need <= 2) return go(IntTag<2>{});
    if (pl.need <= 4) return go(IntTag<4>{});
    if (pl.need <= 6) return go(IntTag<6>{});
    if (pl.need <= 10) return go(IntTag<10>{});
    if (pl.need <= 14) return go(IntTag<14>{});
    if (pl.need <= 18) return go(IntTag<18>{});
    if (pl.need <= 26) return go(IntTag<26>{});
    return go(IntTag<kResMaxNP>{});
}

template <typename InT, int STAGE>
static hipError_t launch_res_generic(const void* x, void* y, int64_t rows, int64_t width, int64_t out_width, int ch,
                                     const int32_t* hq, int L, int U, int D, int phase, int frac, int acc_bits,
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
        FIR_LAUNCH((fir1d_resample_generic_kernel<InT, STAGE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, out_width, (int64_t)ch, (int64_t)U, (int64_t)D,
                           (int64_t)phase, td, L, frac, acc_bits);
    else
        FIR_LAUNCH((fir1d_resample_generic_kernel<InT, STAGE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, out_width, (int64_t)ch, (int64_t)U, (int64_t)D,
                           (int64_t)phase, td, L, frac, acc_bits);
    return hipGetLastError();
}

int launch_fir1d_resample(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                          int up, int decim, int phase, int frac, int acc_bits, int stage, void* y, hipStream_t stream,
                          std::string* err) {
    int64_t ow = 0;
    const int rc = check_fir1d_resample(in_dtype, rows, width, ch, hq, L, up, decim, phase, frac, acc_bits, stage, &ow,
                                        err);
    if (rc) return rc;
    if (rows == 0 || ow == 0) return FIR_OK;
    if (!x || !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    // U = 1 and D = 1 are the decimator and the interpolator by definition, and those are tuned
    if (up == 1)
        return launch_fir1d_decim(x, in_dtype, rows, width, ch, hq, L, decim, phase, frac, acc_bits, stage, y, stream, err);
    if (decim == 1) return launch_fir1d_interp(x, in_dtype, rows, width, ch, hq, L, up, frac, acc_bits, stage, y, stream, err);
    const bool fast = resample_path_ok(x, in_dtype, rows, width, ch, hq, L, up, decim, frac, acc_bits, ow);
    const hipError_t e = with_io(in_dtype, stage, [&](auto t, auto st) {
        using InT = typename decltype(t)::type;
        if (!fast)
            return launch_res_generic<InT, st>(x, y, rows, width, ow, ch, hq, L, up, decim, phase, frac, acc_bits, stream);
        if constexpr (sizeof(InT) == 2) {
            if (ch == 2)
                return launch_res_ch<InT, st, 2>(x, y, rows, width, ow, hq, L, up, decim, phase, frac, acc_bits, stream);
        }
        return launch_res_ch<InT, st, 1>(x, y, rows, width, ow, hq, L, up, decim, phase, frac, acc_bits, stream);
    });
    if (e != hipSuccess) return *err = std::string("fir1d resample launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace fir
