// capi_cresample.hip — the extern "C" boundary of libfir_cresample.so (declared in include/fir_cresample.h).
//
// The device-pointer entry only enqueues on the caller's stream.  The host-pointer entry refuses
// everything the checks can before it looks at a device, then goes through the host layer the
// extension libraries share (csrc_cext/cext_capi.h: the per-device stream and buffers, the copies,
// the error text, guarded()).
#include "cext_capi.h"
#include "cresample.h"

#ifndef FIR_CRESAMPLE_BUILD_ID
#error "FIR_CRESAMPLE_BUILD_ID is set by the Makefile"
#endif

using cext::fail;
using cext::guarded;

extern "C" {

const char* fir_cresample_build_id(void) { return FIR_CRESAMPLE_BUILD_ID; }

const char* fir_cresample_last_error(void) { return cext::g_err.c_str(); }

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
        const int rc = cresample::check(x, y, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, &ow,
                                        &err);
        if (rc) return fail(rc, err);
        if (rows == 0 || ow == 0)  // nothing to compute: no device is looked at (the launcher records that)
            return cresample::launch(x, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, y,
                                     nullptr, &err);
        const size_t in_bytes = (size_t)(rows * width) * 2 * sizeof(int16_t);
        const size_t out_bytes = (size_t)(rows * ow) * 2 * (out_stage == FIR_OUT_I32 ? 4 : 1);
        return cext::host_rows("libfir_cresample", device, x, y, in_bytes, out_bytes,
                               [&](const int16_t* x_dev, void* y_dev, hipStream_t s, std::string* e) {
                                   return cresample::launch(x_dev, rows, width, hq, taps, up, decim, phase, frac_bits,
                                                            acc_bits, out_stage, y_dev, s, e);
                               });
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
