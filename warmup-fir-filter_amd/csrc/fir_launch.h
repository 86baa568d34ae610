// fir_launch.h — internal launch functions (C++), wrapped by the C ABI in capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "fir_hip.h"

namespace fir {

// The launch record (launch_log.hip): every kernel launch of the library goes through FIR_LAUNCH,
// which (a) lists the kernel in the census -- a registry of every instantiation any site can
// launch, filled while the library loads by Site<K>::reg's initialiser, no launch needed -- and
// (b) when the CALLING THREAD has the log on (fir_launch_log_begin), appends the kernel, grid and
// block to that thread's list.  Off, a launch pays one thread-local flag test.  Names are resolved
// only when a record is read (hipKernelNameRefByPtr + demangling).
bool census_add(const void* kernel);
extern thread_local bool t_launch_log_on;
void launch_log_add(const void* kernel, dim3 grid, dim3 block, const std::string& note);
template <auto K>
struct Site {
    static inline const bool reg = census_add((const void*)K);
};
// The record as text, one line per launch / census entry: name \t grid \t block \t flags \t note
// (census: name \t\t\t flags \t); a bit-mask template argument (the register kernels' FLAGS, the
// 2-D kernels' MODE) is spelled in `flags` by the tables beside the masks' definitions
// (kRegFlagNames, kMode2dNames).  fir_status; FIR_EINVAL with *need = the bytes wanted (NUL
// included) when cap is too small, the record kept.
void launch_log_begin();
int launch_log_end(char* buf, size_t cap, size_t* need, std::string* err);
int kernel_census(char* buf, size_t cap, size_t* need, std::string* err);

// FIR_LAUNCH((kernel<...>), grid, block, shmem, stream, args...): hipLaunchKernelGGL plus the
// record.  FIR_LAUNCH_NOTE takes first a std::string expression, evaluated only when the log is
// on, for what the kernel's form owes to run-time arguments (e.g. "mode=acc32 hs0=3").
#define FIR_LAUNCH_NOTE(note, kernel, grid, block, shmem, stream, ...)                             \
    do {                                                                                           \
        (void)&::fir::Site<(kernel)>::reg;                                                         \
        if (::fir::t_launch_log_on) ::fir::launch_log_add((const void*)(kernel), grid, block, note); \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                       \
    } while (0)
#define FIR_LAUNCH(kernel, grid, block, shmem, stream, ...) \
    FIR_LAUNCH_NOTE(std::string(), kernel, grid, block, shmem, stream, __VA_ARGS__)

// Device copies of host tables (long tap sets, matrix-core tap fragments) on the current device
// (dev_tables.hip): cached by the exact bytes they are made from -- their content, or the inputs
// a derived table is built from, behind a kind tag (table_acquire builds the table with `fill`
// only on a miss) -- looked up by a 128-bit hash of those bytes and confirmed by comparing them
// (a hash collision is a miss, never another table), uploaded once (complete before the call
// returns).  Every acquire is a hold on the table for ONE launch, released by table_release after
// that launch is enqueued on `stream` (TableHold does it at scope exit): the cache frees a table
// only when no hold is outstanding and every launch that used it has completed; a table used
// inside a stream capture is kept for the process life.  nullptr + *err on failure.  The first use
// of a table cannot be captured in a hipGraph (warm up before capturing).
enum TableKind : uint8_t { kTableRaw = 1, kTableMfmaFrag = 2 };
struct TableHash {
    uint64_t a = 0xcbf29ce484222325ull, c = 0x84222325cbf29ce4ull;
    std::vector<uint8_t> src;  // every byte added: the identity the cache compares on a hash hit
    explicit TableHash(TableKind kind) { add_val(kind); }
    void add(const void* p, size_t n);
    template <typename T>
    void add_val(const T& v) { add(&v, sizeof(v)); }
};
const void* table_acquire(TableHash&& h, size_t bytes, const std::function<void(void*)>& fill, std::string* err);
void table_release(const void* d, hipStream_t stream, bool launched = true);
const void* device_table(const void* host, size_t bytes, std::string* err);  // table_acquire by content
struct TableHold {  // one launch's hold: released (its use recorded on `s`) when the scope ends
    const void* p;
    hipStream_t s;
    TableHold(const void* p_, hipStream_t s_) : p(p_), s(s_) {}
    TableHold(const TableHold&) = delete;
    TableHold& operator=(const TableHold&) = delete;
    ~TableHold() { table_release(p, s); }
};

// The check_* functions are the structural checks each launcher runs first, on their own: what a
// host entry refuses before it needs a device (an empty problem passes zero sizes).  fir_status
// and *err, as the launchers.
int check_fir1d(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int F, int frac,
                int acc_bits, int stage, std::string* err);
int check_fir1d_ideal(int64_t rows, int64_t width, const double* h, int L, std::string* err);
int check_fir2d(int64_t frames, int64_t height, int64_t width, const int32_t* hq, int tap_rows, int tap_cols, int frac,
                int acc_bits, int stage, std::string* err);
int check_fir2d_ideal(int64_t frames, int64_t height, int64_t width, const double* h, int tap_rows, int tap_cols,
                      std::string* err);
int check_restore_u8(int64_t n, int policy, std::string* err);

// bytes per sample of a (checked) fir_in_dtype / fir_out_stage
inline size_t in_size(int in_dtype) { return in_dtype == FIR_IN_I16 ? 2 : 1; }
inline size_t out_size(int stage) { return stage == FIR_OUT_I32 ? 4 : 1; }

// Enqueue the row-wise 1-D fixed FIR on `stream`; device pointers.  Returns fir_status.
int launch_fir1d_rows(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                      int frac, int acc_bits, int stage, void* y, hipStream_t stream, std::string* err);

// Long filters (up to 64 taps, one channel, int16 taps, acc_bits <= 32): the LDS-window
// v_dot2 kernel (fir1d_lds.hip).  lds_path_ok says whether it applies.
// Long filters on the matrix cores (fir1d_mfma.hip): 2..64 int16 taps, one channel,
// acc_bits <= 32, one row or rows of a multiple of 8 samples, aligned buffers.
bool mfma_path_ok(const void* x, const void* y, int in_dtype, int64_t rows, int64_t rowlen, int64_t total, int ch,
                  const int32_t* hq, int L, int frac, int acc_bits);
hipError_t launch_fir1d_mfma(const void* x, int in_dtype, int64_t rows, int64_t rowlen, int64_t total,
                             const int32_t* hq, int L, int frac, int acc_bits, int stage, void* y, hipStream_t s);
bool lds_path_ok(const void* x, const void* y, int in_dtype, int64_t rows, int64_t rowlen, int64_t total, int ch,
                 const int32_t* hq, int L, int frac, int acc_bits);
hipError_t launch_fir1d_lds(const void* x, int in_dtype, int64_t rows, int64_t rowlen, int64_t total,
                            const int32_t* hq, int L, int frac, int acc_bits, int stage, void* y, hipStream_t s);

// A no-wrap call (acc_bits >= 64) whose exact sum could reach 2^63: the generic kernels then sum
// in 128 bits (fir1d.hip).
bool needs_wide(int in_dtype, const int32_t* hq, int L, int acc_bits);

// The decimating row-wise FIR (fir1d_decim.hip): y[r, m, c] = y_full[r, m * decim + phase, c] with
// y_full what launch_fir1d_rows gives, rows x decim_out_width x ch outputs.  decim_out_width: -1
// for a bad decim / phase / width.  check_fir1d_decim: check_fir1d's checks, then decim, phase
// and the sizes; *out_width on success.  decim_path_ok: the LDS polyphase v_dot2 kernel applies
// (2 <= decim <= 16, up to 128 int16 taps, acc_bits <= 32, frac <= 31, u8 of one channel or
// int16 of one or two, x aligned as lds_path_ok asks, one row or rows of a multiple of 8
// samples); every other call runs the generic one-output-per-thread kernel.
int64_t decim_out_width(int64_t width, int decim, int phase);
int check_fir1d_decim(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int decim,
                      int phase, int frac, int acc_bits, int stage, int64_t* out_width, std::string* err);
bool decim_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                   int decim, int frac, int acc_bits, int64_t out_width);
int launch_fir1d_decim(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                       int decim, int phase, int frac, int acc_bits, int stage, void* y, hipStream_t stream,
                       std::string* err);

// The interpolating row-wise FIR (fir1d_interp.hip): what launch_fir1d_rows gives for x with
// up - 1 zero frames stuffed after every frame, rows x interp_out_width x ch outputs.
// interp_out_width: width * up, -1 for up < 1, width < 0 or overflow.  check_fir1d_interp:
// check_fir1d's checks, then up and the sizes.  interp_path_ok: the LDS polyphase v_dot2 kernel
// applies (2 <= up <= 16, up to 128 int16 taps, acc_bits <= 32, frac <= 31, u8 of one channel or
// int16 of one or two, x aligned as decim_path_ok asks, one row or rows of a multiple of 8
// samples; y at any element address); every other call runs the generic one-output-per-thread
// kernel.
int64_t interp_out_width(int64_t width, int up);
int check_fir1d_interp(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up, int frac,
                       int acc_bits, int stage, std::string* err);
bool interp_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up,
                    int frac, int acc_bits);
int launch_fir1d_interp(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                        int up, int frac, int acc_bits, int stage, void* y, hipStream_t stream, std::string* err);

// The rational resampling row-wise FIR (fir1d_resample.hip): y[r, m, c] = y_up[r, m * decim + phase, c]
// with y_up what launch_fir1d_interp gives, rows x resample_out_width x ch outputs.
// resample_out_width: decim_out_width(width * up, decim, phase), -1 for a bad up / decim / phase /
// width or a width * up past int64.  check_fir1d_resample: check_fir1d's checks, then up, decim,
// phase and the sizes; *out_width on success.  launch_fir1d_resample forwards up == 1 to
// launch_fir1d_decim and decim == 1 to launch_fir1d_interp.  resample_path_ok: the LDS polyphase
// v_dot2 kernel applies (2 <= up, decim <= 16, int16 taps with at most 64 per phase, acc_bits <= 32,
// frac <= 31, u8 of one channel or int16 of one or two, x aligned as interp_path_ok asks, one row or
// rows of a multiple of 8 samples; y at any element address); every other call runs the generic
// one-output-per-thread kernel.
int64_t resample_out_width(int64_t width, int up, int decim, int phase);
int check_fir1d_resample(int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up, int decim,
                         int phase, int frac, int acc_bits, int stage, int64_t* out_width, std::string* err);
bool resample_path_ok(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L, int up,
                      int decim, int frac, int acc_bits, int64_t out_width);
int launch_fir1d_resample(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq, int L,
                          int up, int decim, int phase, int frac, int acc_bits, int stage, void* y, hipStream_t stream,
                          std::string* err);

// The complex-coefficient row-wise FIR for complex int16 (fir1d_cplx.hip): x rows x width frames
// of interleaved (re, im) int16, hq L x 2 int32 (hr[k], hi[k]), y rows x width x 2 outputs of the
// stage's type.  check_fir1d_cplx: check_fir1d's checks for int16 of two channels, then the sizes.
// launch_fir1d_cplx forwards taps whose every hi is 0 to launch_fir1d_rows with channels = 2.
// cplx_path_ok: the LDS sliding-window v_dot2 kernel applies (up to 64 taps with both parts in
// [-32767, 32767], acc_bits <= 32, frac <= 31, FIR_OUT_I32, x and y 16-byte aligned, one row or
// rows of a multiple of 4 frames); every other call runs the generic one-frame-per-thread kernel.
int check_fir1d_cplx(int64_t rows, int64_t width, const int32_t* hq, int L, int frac, int acc_bits, int stage,
                     std::string* err);
bool cplx_path_ok(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int frac,
                  int acc_bits, int stage);
int launch_fir1d_cplx(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int frac, int acc_bits,
                      int stage, void* y, hipStream_t stream, std::string* err);

// F filters of L taps (hq row-major F x L) over the same x; y = F consecutive output planes.
int launch_fir1d_rows_multi(const void* x, int in_dtype, int64_t rows, int64_t width, int ch, const int32_t* hq,
                            int L, int F, int frac, int acc_bits, int stage, void* y, hipStream_t stream,
                            std::string* err);
// n images, F filters each: output plane (i, f) at planes[i * F + f]; every image is checked
// before anything launches.  u8 -> sat-u8 banks of one channel on the register kernel go out as
// ONE launch per 8 images (and per 4 filters), the rest as launch_fir1d_rows per plane.
int launch_fir1d_images_multi(int n, const void* const* xs, const int64_t* rows, const int64_t* widths, int in_dtype,
                              int ch, const int32_t* hq, int L, int F, int frac, int acc_bits, int stage,
                              void* const* planes, hipStream_t stream, std::string* err);

// Recompute the halo-dependent edge outputs of a single-row segment.
int launch_fir1d_edges(const void* x, int in_dtype, int64_t n, int ch, const int32_t* hq, int L, int frac,
                       int acc_bits, int stage, const void* halo_left, const void* halo_right, void* y,
                       hipStream_t stream, std::string* err);

// A single-row shard with its halos: bulk + edges in one register-kernel launch when possible.
int launch_fir1d_segment(const void* x, int in_dtype, int64_t n, int ch, const int32_t* hq, int L, int frac,
                         int acc_bits, int stage, const void* halo_left, const void* halo_right, void* y,
                         hipStream_t stream, std::string* err);

// Per-step halo ordering for sharded segments (halo_gate.hip): mailbox size, its zeroing, and
// the one-wave gate kernel (publish own edges, wait for both neighbours' epoch, copy their
// edges into the local halo buffers).
int64_t halo_mailbox_bytes(int64_t hl_bytes, int64_t hr_bytes);
int launch_halo_mailbox_init(void* mailbox, int64_t bytes, int64_t hl_bytes, int64_t hr_bytes, hipStream_t stream,
                             std::string* err);
int launch_halo_gate(const void* x, int64_t seg_bytes, int64_t hl_bytes, int64_t hr_bytes, void* mailbox,
                     const void* left_mailbox, const void* right_mailbox, void* halo_left, void* halo_right,
                     int32_t* status, double timeout_s, hipStream_t stream, std::string* err);

// 2-D fixed FIR over `frames` uint8 frames of height x width stored back to back (one launch).
// 2-D u8 -> sat-u8 frames on the int8 matrix cores (fir2d_mfma.hip); hipErrorNotSupported when
// the shape, alignment or taps are outside its cover (the caller then takes fir2d_reg_kernel)
hipError_t launch_fir2d_mfma(const uint8_t* x, int64_t frames, int64_t H, int64_t W, const int32_t* hq, int R, int C,
                             int frac, int acc_bits, int stage, void* y, hipStream_t s);
int launch_fir2d(const uint8_t* x, int64_t frames, int64_t height, int64_t width, const int32_t* hq, int tap_rows,
                 int tap_cols, int frac, int acc_bits, int stage, void* y, hipStream_t stream, std::string* err);

// float64 ideal model over uint8 rows.
int launch_fir1d_ideal(const uint8_t* x, int64_t rows, int64_t width, const double* h, int L, double* y,
                       hipStream_t stream, std::string* err);

// float64 ideal model of the 2-D FIR over `frames` uint8 frames stored back to back (ideal2d.hip).
int launch_fir2d_ideal(const uint8_t* x, int64_t frames, int64_t height, int64_t width, const double* h, int tap_rows,
                       int tap_cols, double* y, hipStream_t stream, std::string* err);

// Fixed-vs-ideal comparison metrics (one pass); `work` >= metrics_work_bytes(n).
size_t metrics_work_bytes(int64_t n);
int metrics_dtype_size(int fixed_dtype);  // bytes per element of a fir_num_dtype, 0 if unknown
int launch_metrics(const double* ideal, const void* fixed, int fixed_dtype, int64_t n, double* out, void* work,
                   hipStream_t stream, std::string* err);

// f64 -> u8 restore conversion (FIR_RESTORE_*); `work` >= restore_work_bytes() for normalize.
size_t restore_work_bytes();
int launch_restore_u8(const double* a, int64_t n, int policy, uint8_t* out, void* work, hipStream_t stream,
                      std::string* err);

}  // namespace fir
