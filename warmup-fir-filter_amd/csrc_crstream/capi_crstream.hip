// capi_crstream.hip — the extern "C" boundary of libfir_crstream.so (declared in include/fir_crstream.h).
//
// The device-pointer entry only enqueues on the caller's stream.  The host-pointer entry refuses
// everything the checks can before it looks at a device, then goes through the host layer the
// extension libraries share (csrc_cext/cext_capi.h: the per-device stream and buffers, the copies,
// the error text, guarded()), in its form for two inputs and two outputs.
#include "cext_capi.h"
#include "crstream.h"

#ifndef FIR_CRSTREAM_BUILD_ID
#error "FIR_CRSTREAM_BUILD_ID is set by the Makefile"
#endif

using cext::fail;
using cext::guarded;

extern "C" {

const char* fir_crstream_build_id(void) { return FIR_CRSTREAM_BUILD_ID; }

const char* fir_crstream_last_error(void) { return cext::g_err.c_str(); }

int64_t fir_cplx_rstream_out_width(int64_t width, int up, int decim, int phase) {
    return crstream::out_width(width, up, decim, phase);
}

int fir_cplx_rstream_next_phase(int64_t width, int up, int decim, int phase) {
    return crstream::next_phase(width, up, decim, phase);
}

int fir_cplx_rstream_hist_frames(int taps, int up) { return crstream::hist_frames(taps, up); }

int fir_cplx_rstream_block_dev(const int16_t* x_dev, const int16_t* hist_in_dev, int64_t rows, int64_t width,
                               const int32_t* hq, int taps, int up, int decim, int phase, int frac_bits, int acc_bits,
                               int out_stage, void* y_dev, int16_t* hist_out_dev, void* stream) {
    return guarded([&]() -> int {
        std::string err;
        const int rc = crstream::launch(x_dev, hist_in_dev, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits,
                                        out_stage, y_dev, hist_out_dev, (hipStream_t)stream, &err);
        return rc ? fail(rc, err) : FIR_OK;
    });
}

int fir_cplx_rstream_block(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq,
                           int taps, int up, int decim, int phase, int frac_bits, int acc_bits, int out_stage, void* y,
                           int16_t* hist_out, int device) {
    return guarded([&]() -> int {
        std::string err;
        int64_t ow = 0;
        const int rc = crstream::check(x, y, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, &ow,
                                       &err);
        if (rc) return fail(rc, err);
        const int64_t H = crstream::hist_frames(taps, up);
        const bool writes_hist = hist_out && H > 0;
        if (rows == 0 || (ow == 0 && !writes_hist))  // nothing to compute or write: no device is looked at
            return crstream::launch(x, hist_in, rows, width, hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage, y,
                                    nullptr, nullptr, &err);
        const size_t in_bytes = (size_t)(rows * width) * 2 * sizeof(int16_t);
        const size_t hist_bytes = (size_t)(rows * H) * 2 * sizeof(int16_t);
        const size_t out_bytes = (size_t)(rows * ow) * 2 * (out_stage == FIR_OUT_I32 ? 4 : 1);
        return cext::host_rows2("libfir_crstream", device, x, in_bytes, H > 0 ? hist_in : nullptr, hist_bytes, y,
                                out_bytes, writes_hist ? hist_out : nullptr, hist_bytes,
                                [&](const int16_t* x_dev, const int16_t* hi_dev, void* y_dev, int16_t* ho_dev,
                                    hipStream_t s, std::string* e) {
                                    return crstream::launch(x_dev, hi_dev, rows, width, hq, taps, up, decim, phase,
                                                            frac_bits, acc_bits, out_stage, y_dev, ho_dev, s, e);
                                });
    });
}

int fir_cplx_rstream_route(uintptr_t x_addr, uintptr_t hist_in_addr, uintptr_t y_addr, uintptr_t hist_out_addr,
                           int64_t rows, int64_t width, const int32_t* hq, int taps, int up, int decim, int phase,
                           int frac_bits, int acc_bits, int out_stage, int* tap_bucket) {
    if (tap_bucket) *tap_bucket = 0;
    int route = -1;
    (void)guarded([&]() -> int {
        std::string err;
        int64_t ow = 0;
        const int rc = crstream::check((const void*)x_addr, (const void*)y_addr, rows, width, hq, taps, up, decim, phase,
                                       frac_bits, acc_bits, out_stage, &ow, &err);
        if (rc) return fail(rc, err);
        int bucket = 0;
        route = rows == 0 || ow == 0 ? (int)FIR_CRSTREAM_NONE
                                     : crstream::route_of(x_addr, hist_in_addr, y_addr, hist_out_addr, rows, width, ow,
                                                          hq, taps, up, decim, phase, frac_bits, acc_bits, out_stage,
                                                          &bucket);
        if (tap_bucket) *tap_bucket = bucket;
        return FIR_OK;
    });
    return route;
}

int fir_cplx_rstream_last_launch(int* route, int* tap_bucket) {
    crstream::last_launch(route, tap_bucket);
    return FIR_OK;
}

}  // extern "C"
