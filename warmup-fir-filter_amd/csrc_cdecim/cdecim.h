// cdecim.h — what capi_cdecim.hip uses of fir1d_cplx_decim.hip (C++, internal to libfir_cdecim.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fir_cdecim.h"

namespace cdecim {

// -1 for a bad decim / phase / width
int64_t out_width(int64_t width, int decim, int phase);

// The checks of the header, 1 to 5, in its order; fir_status and *err.  *ow: the out_width.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase,
          int frac, int acc_bits, int stage, int64_t* ow, std::string* err);

// The one dispatch decision, on checked arguments of a problem that is not empty: a FIR_CDECIM_*
// route and the fast path's tap bucket (0 off it).
int route_of(uintptr_t x, uintptr_t y, int64_t rows, int64_t width, int64_t ow, const int32_t* hq, int L, int decim,
             int frac, int acc_bits, int stage, int* bucket);

// check + route_of + the launch on `stream` of the current device.  Records what it launched for
// last_launch (this thread).
int launch(const int16_t* x, int64_t rows, int64_t width, const int32_t* hq, int L, int decim, int phase, int frac,
           int acc_bits, int stage, void* y, hipStream_t stream, std::string* err);

void last_launch(int* route, int* bucket);

}  // namespace cdecim
