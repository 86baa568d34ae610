// capi_cinterp.hip — the extern "C" boundary of libfir_cinterp.so (declared in include/fir_cinterp.h).
//
// The device-pointer entry only enqueues on the caller's stream.  The host-pointer entry refuses
// everything the checks can before it looks at a device, then goes through the host layer the
// extension libraries share (csrc_cext/cext_capi.h: the per-device stream and buffers, the copies,
// the error text, guarded()).
#include "cext_capi.h"
#include "cinterp.h"

#ifndef FIR_CINTERP_BUILD_ID
#error "FIR_CINTERP_BUILD_ID is set by the Makefile"
#endif

using cext::fail;
using cext::guarded;

extern "C" {

const char* fir_cinterp_build_id(void) { return FIR_CINTERP_BUILD_ID; }

const char* fir_cinterp_last_error(void) { return cext::g_err.c_str(); }

int64_t fir_cplx_interp_out_width(int64_t width, int up) { return cinterp::out_width(width, up); }

int fir_cplx_interp_rows_dev(const int16_t* x_dev, int64_t rows, int64_t width, const int32_t* hq, int taps, int up,
                             int frac_bits, int acc_bits, int out_stage, void* y_dev, void* stream) {
    return guarded([&]() -> int {
        std::string err;
        const int rc = cinterp::launch(x_dev, rows, width, hq, taps, up, frac_bits, acc_bits, out_stage, y_dev,
                                       (hipStream_t)stream, &err);
        return rc ? fail(rc, err) : FIR_OK;
    });
}

int fir_cplx_interp_rows(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int taps, int up,
                         int frac_bits, int acc_bits, int out_stage, void* y, int device) {
    return guarded([&]() -> int {
        std::string err;
        const int rc = cinterp::check(x, y, rows, width, hq, taps, up, frac_bits, acc_bits, out_stage, &err);
        if (rc) return fail(rc, err);
        if (rows == 0 || width == 0)  // nothing to compute: no device is looked at (the launcher records that)
            return cinterp::launch(x, rows, width, hq, taps, up, frac_bits, acc_bits, out_stage, y, nullptr, &err);
        const size_t in_bytes = (size_t)(rows * width) * 2 * sizeof(int16_t);
        const size_t out_bytes = (size_t)(rows * width * up) * 2 * (out_stage == FIR_OUT_I32 ? 4 : 1);
        return cext::host_rows("libfir_cinterp", device, x, y, in_bytes, out_bytes,
                               [&](const int16_t* x_dev, void* y_dev, hipStream_t s, std::string* e) {
                                   return cinterp::launch(x_dev, rows, width, hq, taps, up, frac_bits, acc_bits, out_stage,
                                                          y_dev, s, e);
                               });
    });
}

int fir_cplx_interp_route(uintptr_t x_addr, uintptr_t y_addr, int64_t rows, int64_t width, const int32_t* hq, int taps,
                          int up, int frac_bits, int acc_bits, int out_stage, int* window_bucket) {
    if (window_bucket) *window_bucket = 0;
    int route = -1;
    (void)guarded([&]() -> int {
        std::string err;
        const int rc = cinterp::check((const void*)x_addr, (const void*)y_addr, rows, width, hq, taps, up, frac_bits,
                                      acc_bits, out_stage, &err);
        if (rc) return fail(rc, err);
        int bucket = 0;
        route = rows == 0 || width == 0 ? (int)FIR_CINTERP_NONE
                                        : cinterp::route_of(x_addr, y_addr, rows, width, hq, taps, up, frac_bits,
                                                            acc_bits, out_stage, &bucket);
        if (window_bucket) *window_bucket = bucket;
        return FIR_OK;
    });
    return route;
}

int fir_cplx_interp_last_launch(int* route, int* window_bucket) {
    cinterp::last_launch(route, window_bucket);
    return FIR_OK;
}

}  // extern "C"
