// cstream.h — what capi_cstream.hip uses of fir1d_cplx_stream.hip (C++, internal to libfir_cstream.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fir_cstream.h"

namespace cstream {

// -1 for a bad decim / phase / width
int64_t out_width(int64_t width, int decim, int phase);
int next_phase(int64_t width, int decim, int phase);

// The checks of the header, 1 to 5, in its order; fir_status and *err.  *ow: the out_width.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase,
          int frac, int acc_bits, int stage, int64_t* ow, std::string* err);

// The one dispatch decision, on checked arguments of a call that runs a FIR kernel (rows and ow not
// 0): a FIR_CSTREAM_* route and the fast path's tap bucket (0 off it).  A history address of 0: NULL.
int route_of(uintptr_t x, uintptr_t hist_in, uintptr_t y, uintptr_t hist_out, int64_t rows, int64_t width, int64_t ow,
             const int32_t* hq, int L, int decim, int frac, int acc_bits, int stage, int* bucket);

// check + route_of + the FIR launch and the history launch on `stream` of the current device.
// Records the FIR kernel it launched for last_launch (this thread).
int launch(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq, int L, int decim,
           int phase, int frac, int acc_bits, int stage, void* y, int16_t* hist_out, hipStream_t stream,
           std::string* err);

void last_launch(int* route, int* bucket);

}  // namespace cstream
