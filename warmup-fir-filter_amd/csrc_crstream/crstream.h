// crstream.h — what capi_crstream.hip uses of fir1d_cplx_rstream.hip (C++, internal to libfir_crstream.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fir_crstream.h"

namespace crstream {

// -1 for a bad up / decim / phase / width or a width * up past int64
int64_t out_width(int64_t width, int up, int decim, int phase);
int next_phase(int64_t width, int up, int decim, int phase);
// H = (taps - 1) / up; -1 for taps < 1 or up < 1
int hist_frames(int L, int up);

// The checks of the header, 1 to 4, in its order; fir_status and *err.  *ow: the out_width.
int check(const void* x, const void* y, int64_t rows, int64_t width, const int32_t* hq, int L, int up, int decim,
          int phase, int frac, int acc_bits, int stage, int64_t* ow, std::string* err);

// The one dispatch decision, on checked arguments of a call that runs a FIR kernel (rows and ow not
// 0): a FIR_CRSTREAM_* route and the fast path's tap bucket (0 off it).  A history address of 0: NULL.
int route_of(uintptr_t x, uintptr_t hist_in, uintptr_t y, uintptr_t hist_out, int64_t rows, int64_t width, int64_t ow,
             const int32_t* hq, int L, int up, int decim, int phase, int frac, int acc_bits, int stage, int* bucket);

// check + route_of + the FIR launch and the history launch on `stream` of the current device.
// Records the FIR kernel it launched for last_launch (this thread).
int launch(const int16_t* x, const int16_t* hist_in, int64_t rows, int64_t width, const int32_t* hq, int L, int up,
           int decim, int phase, int frac, int acc_bits, int stage, void* y, int16_t* hist_out, hipStream_t stream,
           std::string* err);

void last_launch(int* route, int* bucket);

}  // namespace crstream
