// fir1d_interp.hip — the interpolating 1-D fixed-point FIR: zero-stuff by U, then filter.
//
//   out_width      = width * U
//   xu[r, i*U, c]  = x[r, i, c], every other frame of xu is 0          (rows x out_width x ch)
//   y              = what fir1d_fixed_rows gives for xu (fir1d.hip): centre L/2, zero padding at
//                    each row's ends, wrap to acc_bits, round-half-up by frac_bits, u8-sat or
//                    int32 stage.  No gain: unity passband gain needs the taps scaled by U.
//
// Polyphase form.  Output j = i*U + e (0 <= e < U) only meets the taps p_e + U*t with
// p_e = (e + L/2) mod U, c_e = (e + L/2) div U:
//
//   acc[r, i*U + e, c] = sum over t >= 0, p_e + U*t < L of hq[p_e + U*t] * x[r, i + c_e - t, c]
//
// p_e and c_e depend on e alone, so a lane that owns input frames and writes all U outputs of
// each uses wave-uniform taps for every one of them.  Two kernels:
//
//  * fir1d_interp_kernel — the hot path (interp_path_ok).  A workgroup owns F consecutive input
//    frames of ONE row (never two rows, so out-of-row samples are zeroed once, at staging):
//    F = 4096 frames of u8, 2048 of int16 (one or two channels), i.e. 4 KiB of input per channel
//    in flight per workgroup.  It works through them as G = F / T tiles of T input frames, T = F
//    halved while the tile's outputs T * U * channels * out_size exceed 16 KiB, but not below 256
//    (int16 -> int32: T = 2048, 1024, 512, 256 at U = 2, 4, 8, 16; complex: half of that, 256 from
//    U = 8 on; u8 -> u8: 4096 up to U = 4, ..., 1024 at U = 16).  A tile is computed in passes of
//    512 frames: lane u owns input frames 2u and 2u + 1 of every pass and produces their 2U
//    consecutive output frames (a tile of 256 frames is half a pass: two waves compute).
//
//    Input.  The workgroup stages the frames behind all of its outputs (whole 8-frame chunks, all
//    of a thread's loads issued before its first LDS write: 16 bytes of int16, 8 bytes of u8
//    widened by v_perm, two 16-byte loads of complex int16 split into an I and a Q plane) as
//    int16 pairs in a LINEAR LDS window per channel.  The window behind all 2U outputs of a lane
//    is frames [2u + S, 2u + 1 + hi] with S = the lowest c_e - n_e + 1 floored to an even frame
//    and hi the highest c_e (n_e = taps of phase e): NP = (hi - S + 2) / 2 pairs, about
//    L / (2U) + 1.  The lane reads its NP + 1 dwords once per pass and channel (lane stride one
//    dword: conflict free for ds_read_b32) and reuses them for every phase; the odd frame's pairs
//    come from one v_alignbit each.  Taps: per phase the sub-filter in window order, zero padded
//    to the bucket NP, as int16 pairs passed BY VALUE (U * NP dwords, read with scalar loads at
//    the phase's offset): no device table, nothing allocated, so the call can be captured in a
//    graph.  Arithmetic: NP v_dot2_i32_i16 per output (wrap-around, no clamp), round32,
//    stage_out32.
//
//    Output.  A lane's outputs are 2U * out_size * channels bytes, so per-lane stores would leave
//    the lanes of one store instruction that far apart.  Every result goes to an LDS output stage
//    instead, at the byte it has in the tile's output run, and the workgroup then writes that run
//    as whole 16-byte vectors, consecutive lanes consecutive vectors (1 KiB per store
//    instruction).  The stage starts (y address mod 16) bytes in, so LDS vectors and global
//    vectors line up for ANY y address and row length; the partial vector at either end of a tile
//    goes out element by element, inside the tile's own bytes.  Bank layout: byte b of the stage
//    lives at b + 4 * (b / 128), one pad dword per 32, which spreads the lanes' writes (2U *
//    channels elements apart) and the read-back (four dwords per lane) over the banks: conflict
//    free for int32 of one channel at U = 2, 4, 8, 16, two-way for complex int32 at U = 16.
//
//    The tile is as large as the 16 KiB allow so that a tile costs two barriers whatever U is and
//    every thread has stores to issue (measured, profiles/interp: with 512-frame tiles a u8 -> u8
//    tile at U = 2 was 1 KiB of output, one store instruction of one wave between two barriers).
//
//    LDS per workgroup: channels * (F + 2 NP + 13) * 2 bytes of input rounded to chunks (at most
//    8.4 KiB), plus T * U * channels * out_size + 16 bytes of output stage with its padding: 16.5
//    KiB, more only where T = 256 is the floor (int32 at U > 8: up to 33.0 KiB for complex at
//    U = 16): six workgroups per CU as a rule, three in the worst case.
//
//  * fir1d_interp_generic_kernel — every other legal call (any U >= 1, any L up to FIR_MAX_TAPS,
//    any channel count or alignment, acc_bits of any width): one output per thread, walking
//    k = p_e, p_e + U, ... inside the row, taps from a cached device table, exact 64-bit sums
//    (128-bit when needs_wide says so for the whole tap set: conservative and exact).
#include <string>
#include <type_traits>

#include "fir_common.h"
#include "fir_dispatch.h"
#include "fir_launch.h"

namespace fir {

constexpr int kIntInBytes = 4096;     // input frames per workgroup F = G * T: 4096 of u8, 2048 of int16 ...
__host__ __device__ constexpr int int_frames(int in_size) { return kIntInBytes / in_size; }  // ... one or two channels
constexpr int kIntPass = 512;         // input frames per pass of the workgroup: 2 per lane
constexpr int kIntMinT = 256;         // the smallest tile: half a pass, two waves compute
constexpr int kIntOutBytes = 16384;   // T = F halved while T * U * channels * out_size exceeds this
constexpr int kIntMaxU = 16;
constexpr int kIntMaxTaps = 128;
constexpr int kIntMaxNP = 34;         // the largest pair bucket (U = 2, L = 128: 33 pairs)
constexpr int kIntChunk = 8;          // frames per staging step of one thread

// chunks a workgroup stages: lead + its tiles' frames + the last lane's window (2 NP frames more)
__host__ __device__ constexpr int int_chunks(int lead, int frames, int NP) {
    return (lead + frames + 2 * NP + kIntChunk - 1) / kIntChunk;
}
// staging steps per thread: 3 of u8, 2 of int16
__host__ __device__ constexpr int int_steps(int in_size) {
    return (int_chunks(6, int_frames(in_size), kIntMaxNP) + kBlock - 1) / kBlock;
}
static_assert(int_steps(1) == 3 && int_steps(2) == 2, "staging steps");

// the output stage: logical byte b at b + 4 * (b / 128)
__host__ __device__ constexpr uint32_t int_phys(uint32_t b) { return b + ((b >> 7) << 2); }

typedef uint32_t int_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t int_u2 __attribute__((ext_vector_type(2)));

template <int NP>
struct TapsInt {
    uint32_t pk[kIntMaxU * NP];  // phase e, pair p at e * NP + p: (g_e[2p], g_e[2p+1]) in window order
};

template <typename InT, int STAGE, int CH, int NP>
__global__ __launch_bounds__(kBlock) void fir1d_interp_kernel(const InT* __restrict__ x,
                                                              typename OutTraits<STAGE>::T* __restrict__ y,
                                                              int64_t width, uint32_t groups, int U, int T, int S,
                                                              int PL, TapsInt<NP> taps, int shl, int frac) {
    using OutT = typename OutTraits<STAGE>::T;
    constexpr int OS = (int)sizeof(OutT);
    constexpr int F = int_frames((int)sizeof(InT));
    constexpr int kIntMaxIt = int_steps((int)sizeof(InT));
    extern __shared__ __attribute__((aligned(16))) uint32_t int_lds[];  // CH planes of PL dwords, then the output stage
    const uint32_t tb = blockIdx.x % groups;
    const int64_t r = blockIdx.x / groups;
    const int64_t i0 = (int64_t)tb * F;  // first input frame of the workgroup
    const int64_t left = width - i0;
    const int nf = left < F ? (int)left : F;  // its frames (the row's last workgroup: fewer)
    const int gt = (nf + T - 1) / T;                            // its tiles
    const int64_t a0 = i0 + S;                                  // its first window's first frame (even, may be < 0)
    const int64_t o = a0 & ~(int64_t)(kIntChunk - 1);           // LDS origin: floor to 8 frames
    const int lead = (int)(a0 - o);                             // even, 0..6
    const int nchunks = int_chunks(lead, gt * T, NP);
    const InT* __restrict__ xr = x + r * width * CH;

    // ---- stage frames [o, o + 8 * nchunks) of the row (zero outside [0, width)): first every load
    // of the thread, as the raw dwords of memory, then the widening / channel split and the LDS writes
    constexpr int NR = kIntChunk * CH * (int)sizeof(InT) / 4;  // raw dwords per chunk
    constexpr int EP = 4 / (int)sizeof(InT);                   // samples per raw dword
    uint32_t raw[kIntMaxIt][NR];
#pragma unroll
    for (int it = 0; it < kIntMaxIt; ++it) {
        const int k = threadIdx.x + it * kBlock;
        if (k >= nchunks) break;
        const int64_t f = o + (int64_t)k * kIntChunk;
        if (f >= 0 && f + kIntChunk <= width) {
            if constexpr (NR == 2) {
                const int_u2 q = *reinterpret_cast<const int_u2*>(xr + f);
                raw[it][0] = q.x;
                raw[it][1] = q.y;
            } else {
#pragma unroll
                for (int j = 0; j < NR / 4; ++j) {
                    const int_u4 q = reinterpret_cast<const int_u4*>(xr + f * CH)[j];
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
    for (int it = 0; it < kIntMaxIt; ++it) {
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
#pragma unroll
            for (int c = 0; c < CH; ++c) int_lds[c * PL + 4 * k + i] = wv[c];
        }
    }
    __syncthreads();

    uint32_t* const outw = int_lds + CH * PL;
    uint8_t* const outb = reinterpret_cast<uint8_t*>(outw);
    const int u = threadIdx.x;
    const int64_t out_width = width * U;
    for (int g = 0; g < gt; ++g) {
        const int64_t ig = i0 + (int64_t)g * T;  // the tile's first input frame
        const int nv = width - ig < T ? (int)(width - ig) : T;  // its frames inside the row
        char* const yt = reinterpret_cast<char*>(y + (r * out_width + ig * U) * CH);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(yt) & 15u);  // the stage's first byte

        // ---- lane u: the 2U outputs of input frames 2u and 2u + 1 of every pass (kIntPass frames
        // of the tile; a tile of kIntMinT frames is half a pass), into the stage
        const uint32_t estep = (uint32_t)(CH * OS);      // bytes from phase e to e + 1
        const uint32_t fstep = (uint32_t)U * estep;      // ... from a frame to the next
        for (int fp = 2 * u; fp < T && fp < nv; fp += kIntPass) {  // fp: the lane's even frame in the tile
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                uint32_t d[NP + 1], od[NP];
                const int wb = c * PL + (lead + g * T + fp) / 2;
#pragma unroll
                for (int p = 0; p < NP + 1; ++p) d[p] = int_lds[wb + p];
#pragma unroll
                for (int p = 0; p < NP; ++p) od[p] = __builtin_amdgcn_alignbit(d[p + 1], d[p], 16);
                uint32_t b = sh + (uint32_t)fp * fstep + (uint32_t)(c * OS);  // frame fp, phase 0
                for (int e = 0; e < U; ++e, b += estep) {
                    const uint32_t* __restrict__ tp = taps.pk + e * NP;  // wave-uniform
                    uint32_t acc0 = 0, acc1 = 0;
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        acc0 = dot2_acc(d[p], tp[p], acc0);
                        acc1 = dot2_acc(od[p], tp[p], acc1);
                    }
                    const OutT q0 = stage_out32<STAGE>(round32(acc0, shl, frac));
                    const OutT q1 = stage_out32<STAGE>(round32(acc1, shl, frac));
                    if constexpr (OS == 4) {
                        outw[int_phys(b) >> 2] = (uint32_t)q0;
                        outw[int_phys(b + fstep) >> 2] = (uint32_t)q1;
                    } else {
                        outb[int_phys(b)] = q0;
                        outb[int_phys(b + fstep)] = q1;
                    }
                }
            }
        }
        __syncthreads();

        // ---- the tile's output run [sh, end) of the stage, as 16-byte vectors at 16-byte addresses
        const uint32_t end = sh + (uint32_t)nv * (uint32_t)U * (uint32_t)(CH * OS);
        const uint32_t nvec = (end + 15u) >> 4;
        for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) {
            const uint32_t lo = 16u * v;
            if (lo >= sh && lo + 16u <= end) {
                int_u4 q;
                q.x = outw[int_phys(lo) >> 2];
                q.y = outw[int_phys(lo + 4) >> 2];
                q.z = outw[int_phys(lo + 8) >> 2];
                q.w = outw[int_phys(lo + 12) >> 2];
                *reinterpret_cast<int_u4*>(yt - sh + lo) = q;
            } else {  // the partial vector at either end of the run
                const uint32_t b0 = lo < sh ? sh : lo, b1 = lo + 16u < end ? lo + 16u : end;
                for (uint32_t b = b0; b < b1; b += OS) {
                    if constexpr (OS == 4)
                        *reinterpret_cast<uint32_t*>(yt - sh + b) = outw[int_phys(b) >> 2];
                    else
                        *reinterpret_cast<uint8_t*>(yt - sh + b) = outb[int_phys(b)];
                }
            }
        }
        __syncthreads();  // the next tile overwrites the stage
    }
}

// One output per thread: output gi = ((r * out_width + j) * ch + c), j = i * U + e, sums the taps
// p_e + U * t whose sample i + c_e - t lies in row r (the in-row test as loop bounds).
template <typename InT, int STAGE, bool WIDE>
__global__ __launch_bounds__(kBlock) void fir1d_interp_generic_kernel(const InT* __restrict__ x,
                                                                      typename OutTraits<STAGE>::T* __restrict__ y,
                                                                      int64_t n_out, int64_t width, int64_t ch, int64_t U,
                                                                      const int32_t* __restrict__ taps, int L, int frac,
                                                                      int acc_bits) {
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_out) return;
    const int64_t out_width = width * U;
    const int64_t c = gi % ch, q = gi / ch;
    const int64_t j = q % out_width, r = q / out_width;
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

int64_t interp_out_width(int64_t width, int up) {
    int64_t ow = 0;
    if (width < 0 || up < 1 || __builtin_mul_overflow(width, (int64_t)up, &ow)) return -1;
    return ow;
}

int check_fir1d_interp(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up, int frac,
                       int acc_bits, int stage, std::string* err) {
    const int rc = check_fir1d(in_dtype, rows, width, ch, hq, L, 1, frac, acc_bits, stage, err);
    if (rc) return rc;
    if (up < 1) return *err = "up must be >= 1", FIR_EINVAL;
    int64_t rw = 0, n = 0, nu = 0;
    if (__builtin_mul_overflow(rows, width, &rw) || __builtin_mul_overflow(rw, (int64_t)up, &n) ||
        __builtin_mul_overflow(n, (int64_t)ch, &nu) || nu > INT64_MAX / 4)
        return *err = "rows * width * up * channels outputs do not fit in int64 bytes", FIR_EINVAL;
    return FIR_OK;
}

// The windows of the U phases: *S the first frame (relative to the output's input frame, floored
// to even) of the window all phases share, returns its pairs NP.
static int interp_window(int L, int U, int* S) {
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
    *S = lo - (lo & 1);
    return (hi - *S + 2) / 2;
}

// input frames per tile: the workgroup's frames, halved while the tile's outputs exceed kIntOutBytes
static int interp_tile(int frames, int U, int ch, int stage) {
    int T = frames;
    while (T > kIntMinT && T * U * ch * (int)out_size(stage) > kIntOutBytes) T /= 2;
    return T;
}

bool interp_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up,
                    int frac, int acc_bits) {
    if (up < 2 || up > kIntMaxU || L > kIntMaxTaps || acc_bits > 32 || frac > 31) return false;
    if (!(ch == 1 || (ch == 2 && in_dtype == FIR_IN_I16))) return false;
    for (int k = 0; k < L; ++k)
        if (hq[k] < -32768 || hq[k] > 32767) return false;
    const int64_t rowlen = width * ch;
    if ((uintptr_t)x % (in_dtype == FIR_IN_U8 ? 8 : 16) != 0) return false;
    if (!(rows == 1 || rowlen % 8 == 0)) return false;  // every row starts as x does
    const int64_t frames = int_frames((int)in_size(in_dtype));
    const int64_t groups = (width + frames - 1) / frames;
    // the grid is rows * groups workgroups; the kernel holds a group index in 32 bits
    return width < ((int64_t)1 << 40) && groups < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31) / groups;
}

template <typename InT, int STAGE, int CH, int NP>
static hipError_t launch_interp_np(const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int U,
                                   int S, int frac, int acc_bits, hipStream_t s) {
    TapsInt<NP> taps = {};
    for (int e = 0; e < U; ++e) {
        const int pe = (e + L / 2) % U, ce = (e + L / 2) / U;
        const int ne = pe < L ? (L - pe + U - 1) / U : 0;
        int32_t g[2 * NP] = {};  // g[k]: the tap of frame S + k, i.e. t = ce - S - k
        for (int k = 0; k < 2 * NP; ++k) {
            const int t = ce - S - k;
            if (t >= 0 && t < ne) g[k] = hq[pe + U * t];
        }
        for (int p = 0; p < NP; ++p)
            taps.pk[e * NP + p] = ((uint32_t)g[2 * p] & 0xFFFFu) | ((uint32_t)g[2 * p + 1] << 16);
    }
    using OutT = typename OutTraits<STAGE>::T;
    constexpr int F = int_frames((int)sizeof(InT));
    const int T = interp_tile(F, U, CH, STAGE);
    const int PL = int_chunks(6, F, NP) * 4;  // dwords per channel plane (lead <= 6)
    const uint32_t stage_bytes = (uint32_t)(T * U * CH) * (uint32_t)sizeof(OutT) + 16u;
    const size_t lds = (size_t)CH * PL * sizeof(uint32_t) + int_phys(stage_bytes) + 4;
    const int64_t groups = (width + F - 1) / F;
    FIR_LAUNCH((fir1d_interp_kernel<InT, STAGE, CH, NP>), dim3((unsigned)(rows * groups)), dim3(kBlock), lds, s,
                       (const InT*)x, (OutT*)y, width, (uint32_t)groups, U, T, S, PL, taps, 32 - acc_bits, frac);
    return hipGetLastError();
}

template <typename InT, int STAGE, int CH>
static hipError_t launch_interp_ch(const void* x, void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int U,
                                   int frac, int acc_bits, hipStream_t s) {
    int S = 0;
    const int need = interp_window(L, U, &S);
    const auto go = [&](auto np) {
        return launch_interp_np<InT, STAGE, CH, decltype(np)::value>(x, y, rows, width, hq, L, U, S, frac, acc_bits, s);
    };
    if (need <= 2) return go(IntTag<2>{});
    if (need <= 3) return go(IntTag<3>{});
    if (need <= 4) return go(IntTag<4>{});
    if (need <= 6) return go(IntTag<6>{});
    if (need <= 10) return go(IntTag<10>{});
    if (need <= 18) return go(IntTag<18>{});
    return go(IntTag<kIntMaxNP>{});
}

template <typename InT, int STAGE>
static hipError_t launch_interp_generic(const void* x, void* y, int64_t rows, int64_t width, int ch, const int32_t* hq,
                                        int L, int U, int frac, int acc_bits, hipStream_t s) {
    using OutT = typename OutTraits<STAGE>::T;
    const int64_t n_out = rows * width * U * ch;
    const int64_t blocks = (n_out + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    std::string err;
    const int32_t* td = (const int32_t*)device_table(hq, sizeof(int32_t) * (size_t)L, &err);
    if (!td) return hipErrorOutOfMemory;
    TableHold hold(td, s);
    if (needs_wide(sizeof(InT) == 1 ? FIR_IN_U8 : FIR_IN_I16, hq, L, acc_bits))
        FIR_LAUNCH((fir1d_interp_generic_kernel<InT, STAGE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, (int64_t)ch, (int64_t)U, td, L, frac, acc_bits);
    else
        FIR_LAUNCH((fir1d_interp_generic_kernel<InT, STAGE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                           (const InT*)x, (OutT*)y, n_out, width, (int64_t)ch, (int64_t)U, td, L, frac, acc_bits);
    return hipGetLastError();
}

int launch_fir1d_interp(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                        int up, int frac, int acc_bits, int stage, void* y, hipStream_t stream, std::string* err) {
    const int rc = check_fir1d_interp(in_dtype, rows, width, ch, hq, L, up, frac, acc_bits, stage, err);
    if (rc) return rc;
    if (rows == 0 || width == 0) return FIR_OK;
    if (!x || !y) return *err = "x and y must not be NULL", FIR_EINVAL;
    const bool fast = interp_path_ok(x, in_dtype, rows, width, ch, hq, L, up, frac, acc_bits);
    const hipError_t e = with_io(in_dtype, stage, [&](auto t, auto st) {
        using InT = typename decltype(t)::type;
        if (!fast) return launch_interp_generic<InT, st>(x, y, rows, width, ch, hq, L, up, frac, acc_bits, stream);
        if constexpr (sizeof(InT) == 2) {
            if (ch == 2) return launch_interp_ch<InT, st, 2>(x, y, rows, width, hq, L, up, frac, acc_bits, stream);
        }
        return launch_interp_ch<InT, st, 1>(x, y, rows, width, hq, L, up, frac, acc_bits, stream);
    });
    if (e != hipSuccess) return *err = std::string("fir1d interp launch failed: ") + hipGetErrorString(e), FIR_EHIP;
    return FIR_OK;
}

}  // namespace fir
