// cext_capi.h — the host layer behind the extern "C" boundary of an extension library
// (capi_cdecim.hip, capi_cinterp.hip, capi_cresample.hip, capi_cstream.hip, capi_crstream.hip).  No library compiles
// this directory on its own; each includes this header into its one capi_*.hip.
//
// The host-pointer entry owns, per device, one non-blocking stream and a grow-only pair of device
// buffers behind a mutex (calls are serialised per device): H2D copy, kernel, D2H copy, stream
// synchronise, and the calling thread's current device put back.  No C++ exception crosses the
// boundary: every entry that can allocate runs inside guarded().
//
// Everything here has internal linkage (an unnamed namespace): the libraries are loaded into one
// process and each keeps its own error text, device states, streams and buffers.  Nothing `inline`
// with external linkage may be added: it would become one weak dynamic symbol common to all of them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fir_hip.h"

namespace cext {
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

// `lib`: the library's name for the refusal of another architecture ("libfir_cdecim")
int init_locked(DeviceState* st, int device, const char* lib) {
    if (st->init) return FIR_OK;
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(FIR_ENODEV, std::string("device ") + std::to_string(device) + " is " + p.gcnArchName + "; " + lib +
                                    " is built for gfx950 (MI355X) only");
    if (!st->stream) HIP_TRY(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    st->init = true;
    return FIR_OK;
}

// The host-pointer entry of a problem that passed its checks and is not empty: x (in_bytes) goes to
// `device`, launch(x_dev, y_dev, stream, &err) -> fir_status enqueues the kernel, y (out_bytes)
// comes back, and the call returns once the stream has drained.
template <typename Launch>
int host_rows(const char* lib, int device, const void* x, void* y, size_t in_bytes, size_t out_bytes, Launch launch) {
    int rc;
    DeviceRestore restore;
    DeviceState* st = nullptr;
    if ((rc = device_state(device, &st))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    if ((rc = init_locked(st, device, lib))) return rc;
    if ((rc = ensure(st->in, in_bytes)) || (rc = ensure(st->out, out_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(st->in.ptr, x, in_bytes, hipMemcpyHostToDevice, st->stream));
    std::string err;
    rc = launch((const int16_t*)st->in.ptr, st->out.ptr, st->stream, &err);
    if (rc) {  // what is already queued must finish first: the next call reuses the buffers
        (void)hipStreamSynchronize(st->stream);
        return fail(rc, err);
    }
    const hipError_t e = hipMemcpyAsync(y, st->out.ptr, out_bytes, hipMemcpyDeviceToHost, st->stream);
    const hipError_t es = hipStreamSynchronize(st->stream);
    if (e != hipSuccess) return fail(FIR_EHIP, std::string("hipMemcpyAsync (D2H): ") + hipGetErrorString(e));
    if (es != hipSuccess) return fail(FIR_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
    return FIR_OK;
}

// The same for an entry that moves two inputs and two outputs (capi_cstream.hip, capi_crstream.hip: a block and its
// history in, the kept frames and the next history out).  Either second pointer may be NULL: that
// array is not moved and launch gets NULL for it.  The second array of each pair sits in the same
// device buffer as the first, at the next multiple of 256 bytes.
template <typename Launch>
int host_rows2(const char* lib, int device, const void* x, size_t in_bytes, const void* x2, size_t in2_bytes, void* y,
               size_t out_bytes, void* y2, size_t out2_bytes, Launch launch) {
    int rc;
    DeviceRestore restore;
    DeviceState* st = nullptr;
    if ((rc = device_state(device, &st))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    if ((rc = init_locked(st, device, lib))) return rc;
    const size_t in2_at = (in_bytes + 255) / 256 * 256, out2_at = (out_bytes + 255) / 256 * 256;
    if ((rc = ensure(st->in, in2_at + (x2 ? in2_bytes : 0))) || (rc = ensure(st->out, out2_at + (y2 ? out2_bytes : 0))))
        return rc;
    char* const in2 = x2 ? (char*)st->in.ptr + in2_at : nullptr;
    char* const out2 = y2 ? (char*)st->out.ptr + out2_at : nullptr;
    if (in_bytes) HIP_TRY(hipMemcpyAsync(st->in.ptr, x, in_bytes, hipMemcpyHostToDevice, st->stream));
    if (in2 && in2_bytes) HIP_TRY(hipMemcpyAsync(in2, x2, in2_bytes, hipMemcpyHostToDevice, st->stream));
    std::string err;
    rc = launch((const int16_t*)st->in.ptr, (const int16_t*)in2, st->out.ptr, (int16_t*)out2, st->stream, &err);
    if (rc) {  // what is already queued must finish first: the next call reuses the buffers
        (void)hipStreamSynchronize(st->stream);
        return fail(rc, err);
    }
    hipError_t e = hipSuccess;
    if (out_bytes) e = hipMemcpyAsync(y, st->out.ptr, out_bytes, hipMemcpyDeviceToHost, st->stream);
    if (e == hipSuccess && out2 && out2_bytes)
        e = hipMemcpyAsync(y2, out2, out2_bytes, hipMemcpyDeviceToHost, st->stream);
    const hipError_t es = hipStreamSynchronize(st->stream);
    if (e != hipSuccess) return fail(FIR_EHIP, std::string("hipMemcpyAsync (D2H): ") + hipGetErrorString(e));
    if (es != hipSuccess) return fail(FIR_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
    return FIR_OK;
}

#undef HIP_TRY

}  // namespace
}  // namespace cext
