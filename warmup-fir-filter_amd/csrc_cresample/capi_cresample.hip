// capi_cresample.hip — the extern "C" boundary of libfir_cresample.so (declared in include/fir_cresample.h).
//
// The device-pointer entry only enqueues on the caller's stream.  The host-pointer entry owns, per
// device, one non-blocking stream and a grow-only pair of device buffers behind a mutex (calls are
// serialised per device): H2D copy, kernel, D2H copy, stream synchronise, and the calling thread's
// current device put back.  It refuses everything the checks can before it looks at a device.  No
// C++ exception crosses the boundary: every entry that can allocate runs inside guarded().
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "cresample.h"

#ifndef FIR_CRESAMPLE_BUILD_ID
#error "FIR_CRESAMPLE_BUILD_ID is set by the Makefile"
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

template <typename Fn>
int guarded(Fn fn) {
    try {
        return fn();
    } catch (const std::exception& ex) {
        return fail(FIR_EHIP, std::string("internal error: ") + ex.what());
    } catch (...) {
        return fail(FIR_EHIP, "internal error");
    }
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(FIR_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct DeviceBuf {
    void* ptr = nullptr;
    size_t cap = 0;
};

struct DeviceState {
    std::mutex mu;
    bool init = false;
    hipStream_t stream = nullptr;
    DeviceBuf in, out;
};

std::mutex g_devs_mu;
std::vector<std::unique_ptr<DeviceState>> g_devs;

int ensure(DeviceBuf& b, size_t bytes) {
    if (bytes <= b.cap) return FIR_OK;
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.cap = 0;
    const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    const hipError_t e = hipMalloc(&b.ptr, want);
    if (e != hipSuccess) {
        b.ptr = nullptr;
        return fail(FIR_ENOMEM, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    }
    b.cap = want;
    return FIR_OK;
}

// Puts the calling thread's current device back on scope exit.
struct DeviceRestore {
    int prev = -1;
    DeviceRestore() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceRestore() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Validates `device`, makes it current, and returns its state (locked and initialised by the caller).
int device_state(int device, DeviceState** out) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(FIR_ENODEV, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "0 devices"));
    if (device < 0 || device >= n)
        return fail(FIR_ENODEV, "device " + std::to_string(device) + " out of range (" + std::to_string(n) + " devices)");
    {
        std::lock_guard<std::mutex> lk(g_devs_mu);
        while ((int)g_devs.size() < n) g_devs.emplace_back(new DeviceState());
        *out = g_devs[device].get();
    }
    HIP_TRY(hipSetDevice(device));
    return FIR_OK;
}

int init_locked(DeviceState* st, int device) {
    if (st->init) return FIR_OK;
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(FIR_ENODEV, std::string("device ") + std::to_string(device) + " is " + p.gcnArchName +
                                    "; libfir_cresample is built for gfx950 (MI355X) only");
    if (!st->stream) HIP_TRY(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    st->init = true;
    return FIR_OK;
}

}  // namespace

extern "C" {

const char* fir_cresample_build_id(void) { return FIR_CRESAMPLE_BUILD_ID; }

const char* fir_cresample_last_error(void) { return g_err.c_str(); }

int64_t fir_cplx_resample_out_width(int64_t width, int up, int decim, int phase) {
    return cresample::out_width(width, up, decim, phase);
}

int fir_cplx_resample_rows_dev(const int16_t* x_dev, int64_t rows, int64_t width, const int32_t* hq, int taps, int up,
                               int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y_dev,
                               void* stream) {
    return guarded([&]() -> int {
        std::string err;
        const int rc = cresample::launch(x_dev, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage,
                                         y_dev, (hipStream_t)stream, &err);
        return rc ? fail(rc, err) : FIR_OK;
    });
}

int fir_cplx_resample_rows(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int taps, int up, int decim,
                           int phase, int frac_bits, int acc_bits, int out_stage, void* y, int device) {
    return guarded([&]() -> int {
        std::string err;
        int64_t ow = 0;
        int rc = cresample::check(x, y, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, &ow, &err);
        if (rc) return fail(rc, err);
        if (rows == 0 || ow == 0)  // nothing to compute: no device is looked at (the launcher records that)
            return cresample::launch(x, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, y,
                                     nullptr, &err);
        DeviceRestore restore;
        DeviceState* st = nullptr;
        if ((rc = device_state(device, &st))) return rc;
        std::lock_guard<std::mutex> lk(st->mu);
        if ((rc = init_locked(st, device))) return rc;
        const size_t in_bytes = (size_t)(rows * width) * 2 * sizeof(int16_t);
        const size_t out_bytes = (size_t)(rows * ow) * 2 * (out_stage == FIR_OUT_I32 ? 4 : 1);
        if ((rc = ensure(st->in, in_bytes)) || (rc = ensure(st->out, out_bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(st->in.ptr, x, in_bytes, hipMemcpyHostToDevice, st->stream));
        rc = cresample::launch((const int16_t*)st->in.ptr, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits,
                               out_stage, st->out.ptr, st->stream, &err);
        if (rc) {  // what is already queued must finish first: the next call reuses the buffers
            (void)hipStreamSynchronize(st->stream);
            return fail(rc, err);
        }
        const hipError_t e = hipMemcpyAsync(y, st->out.ptr, out_bytes, hipMemcpyDeviceToHost, st->stream);
        const hipError_t es = hipStreamSynchronize(st->stream);
        if (e != hipSuccess) return fail(FIR_EHIP, std::string("hipMemcpyAsync (D2H): ") + hipGetErrorString(e));
        if (es != hipSuccess) return fail(FIR_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
        return FIR_OK;
    });
}

int fir_cplx_resample_route(uintptr_t x_addr, uintptr_t y_addr, int64_t rows, int64_t width, const int32_t* hq, int taps,
                            int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage, int* tap_bucket) {
    if (tap_bucket) *tap_bucket = 0;
    int route = -1;
    (void)guarded([&]() -> int {
        std::string err;
        int64_t ow = 0;
        const int rc = cresample::check((const void*)x_addr, (const void*)y_addr, rows, width, hq, taps, up, decim, phase,
                                        frac_bits, acc_bits, out_stage, &ow, &err);
        if (rc) return fail(rc, err);
        int bucket = 0;
        route = rows == 0 || ow == 0 ? (int)FIR_CRESAMPLE_NONE
                                     : cresample::route_of(x_addr, y_addr, rows, width, ow, hq, taps, up, decim, phase,
                                                           frac_bits, acc_bits, out_stage, &bucket);
        if (tap_bucket) *tap_bucket = bucket;
        return FIR_OK;
    });
    return route;
}

int fir_cplx_resample_last_launch(int* route, int* tap_bucket) {
    cresample::last_launch(route, tap_bucket);
    return FIR_OK;
}

}  // extern "C"
