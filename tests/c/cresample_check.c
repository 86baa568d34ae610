/* cresample_check.c — host AddressSanitizer exercise of the C ABI of libfir_cresample.so
 * (include/fir_cresample.h).
 *
 * Built by `make -C warmup-fir-filter_amd/csrc_cresample asan-check` against a copy of the library
 * whose host code (the checks, the dispatch, the entries) is compiled with
 * -Xarch_host -fsanitize=address; device code is unchanged.  A stand-alone program with its own
 * main: it runs on the CPU, needs no GPU, and launches nothing -- every call here is refused, is
 * empty, or is a query.  Exit status 0 = no failure; ASan aborts on any host memory error. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fir_cresample.h"

static int failures = 0;

static void expect(int cond, const char* what) {
    if (!cond) {
        fprintf(stderr, "FAIL: %s (%s)\n", what, fir_cresample_last_error());
        ++failures;
    }
}

static int said(const char* piece) { return strstr(fir_cresample_last_error(), piece) != NULL; }

#define NO_DEV (1 << 20)

/* the header's tap bucket: the smallest that holds the longest sub-filter n_q */
static int bucket_of(int L, int U, int D, int phase) {
    const int buckets[13] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32};
    int need = 0;
    for (int q = 0; q < U; ++q) {
        const int p = (phase + L / 2 + q * D) % U;
        const int n = p < L ? (L - p + U - 1) / U : 0;
        if (n > need) need = n;
    }
    for (int i = 0; i < 13; ++i)
        if (buckets[i] >= need) return buckets[i];
    return -1;
}

int main(void) {
    const int32_t h3[6] = {1, 2, 3, 4, 5, 6};
    int16_t* x = (int16_t*)calloc(64, sizeof *x); /* heap, so that a stray host access is seen */
    int32_t* y = (int32_t*)calloc(256, sizeof *y);

    /* the build id */
    expect(strlen(fir_cresample_build_id()) == 32, "build id: 32 hex digits");
#ifdef EXPECT_BUILD_ID
    expect(strcmp(fir_cresample_build_id(), EXPECT_BUILD_ID) == 0, "build id: the tree's");
#endif
    expect(strlen(fir_cresample_last_error()) == 0, "no error text before any failure");

    /* out_width */
    for (int U = 1; U <= 17; ++U)
        for (int D = 1; D <= 17; ++D)
            for (int ph = 0; ph < D; ++ph)
                for (int64_t w = 0; w <= 40; ++w) {
                    const int64_t mid = w * U;
                    expect(fir_cplx_resample_out_width(w, U, D, ph) == (mid > ph ? (mid - ph + D - 1) / D : 0), "out_width");
                }
    expect(fir_cplx_resample_out_width(10, 0, 1, 0) == -1 && fir_cplx_resample_out_width(10, 1, 0, 0) == -1 &&
               fir_cplx_resample_out_width(10, 2, 3, 3) == -1 && fir_cplx_resample_out_width(10, 2, 3, -1) == -1 &&
               fir_cplx_resample_out_width(-1, 1, 1, 0) == -1 && fir_cplx_resample_out_width((int64_t)1 << 62, 2, 3, 0) == -1,
           "out_width: bad up / decim / phase / width / product");
    expect(fir_cplx_resample_out_width(INT64_MAX, 1, 1, 0) == INT64_MAX &&
               fir_cplx_resample_out_width(((int64_t)1 << 62) - 1, 2, 1, 0) == INT64_MAX - 1 &&
               fir_cplx_resample_out_width(INT64_MAX, 1, 2, 1) == INT64_MAX / 2,
           "out_width at 2^63 - 1");

    /* the refusals of both entries, in their order */
    for (int host = 0; host < 2; ++host) {
#define CALL(x_, rows, width, hq, taps, U, D, ph, frac, acc, stage, y_)                                      \
    (host ? fir_cplx_resample_rows(x_, rows, width, hq, taps, U, D, ph, frac, acc, stage, y_, NO_DEV)        \
          : fir_cplx_resample_rows_dev(x_, rows, width, hq, taps, U, D, ph, frac, acc, stage, y_, NULL))
        expect(CALL(NULL, -1, 16, NULL, 0, 0, 0, -1, 0, 0, 9, NULL) == FIR_EINVAL && said("out_stage"), "stage first");
        expect(CALL(NULL, -1, 16, NULL, 0, 0, 0, -1, 0, 0, 1, NULL) == FIR_EINVAL && said("rows and width"), "then rows");
        expect(CALL(NULL, 1, 16, NULL, 0, 0, 0, -1, 0, 0, 1, NULL) == FIR_EINVAL && said("hq must not be NULL"), "then hq");
        expect(CALL(NULL, 1, 16, h3, 0, 0, 0, -1, 0, 0, 1, NULL) == FIR_EINVAL && said("taps must be in [1, "), "then taps");
        expect(CALL(NULL, 1, 16, h3, 3, 0, 0, -1, 0, 32, 1, NULL) == FIR_EINVAL && said("frac_bits and acc_bits"), "then frac");
        expect(CALL(NULL, 1, 16, h3, 3, 0, 0, -1, 12, 0, 1, NULL) == FIR_EINVAL && said("frac_bits and acc_bits"), "then acc");
        expect(CALL(NULL, 1, 16, h3, 3, 0, 0, -1, 12, 32, 1, NULL) == FIR_EINVAL && said("up must be >= 1"), "then up");
        expect(CALL(NULL, 1, 16, h3, 3, 3, 0, -1, 12, 32, 1, NULL) == FIR_EINVAL && said("decim must be >= 1"), "then decim");
        expect(CALL(NULL, 1, 16, h3, 3, 3, 2, -1, 12, 32, 1, NULL) == FIR_EINVAL && said("phase must be in [0, decim)"), "then phase");
        expect(CALL(NULL, 1, 16, h3, 3, 3, 2, 2, 12, 32, 1, NULL) == FIR_EINVAL && said("phase must be in [0, decim)"), "phase = decim");
        expect(CALL(NULL, (int64_t)1 << 40, (int64_t)1 << 40, h3, 3, 3, 2, 1, 12, 32, 1, NULL) == FIR_EINVAL && said("must fit in int64"),
               "then the sizes");
        expect(CALL(x, 1, (int64_t)1 << 62, h3, 3, 3, 2, 1, 12, 32, 1, y) == FIR_EINVAL && said("width * up"), "the sizes: width * up");
        expect(CALL(x, (int64_t)1 << 30, (int64_t)1 << 29, h3, 3, 4, 1, 0, 12, 32, 1, y) == FIR_EINVAL && said("rows * out_width * 2 * 4"),
               "the sizes: the output");
        expect(CALL(NULL, 1, 16, h3, 3, 3, 2, 1, 12, 32, 1, NULL) == FIR_EINVAL && said("x and y must not be NULL"), "then NULL x, y");
        expect(CALL(x, 1, 16, h3, 3, 3, 2, 1, 12, 32, 1, NULL) == FIR_EINVAL && said("x and y must not be NULL"), "NULL y");
        /* empty problems: FIR_OK, NULL pointers and all, no device looked at */
        expect(CALL(NULL, 0, 16, h3, 3, 3, 2, 1, 12, 32, 1, NULL) == FIR_OK, "no rows");
        expect(CALL(NULL, 5, 0, h3, 3, 3, 2, 0, 12, 64, 0, NULL) == FIR_OK, "no width");
        expect(CALL(NULL, 0, 0, h3, 3, 1 << 30, 1 << 30, 7, 40, 64, 0, NULL) == FIR_OK, "neither");
        expect(CALL(NULL, 5, 1, h3, 3, 2, 16, 2, 12, 32, 1, NULL) == FIR_OK, "mid_width <= phase");
        expect(CALL(NULL, 5, 5, h3, 3, 3, 16, 15, 12, 32, 1, NULL) == FIR_OK, "mid_width == phase");
        int route = -1, bucket = -1;
        expect(fir_cplx_resample_last_launch(&route, &bucket) == FIR_OK && route == FIR_CRESAMPLE_NONE && bucket == 0,
               "an empty call launched nothing");
#undef CALL
    }
    /* the host form gets as far as the device lookup, and no further */
    expect(fir_cplx_resample_rows(x, 1, 16, h3, 3, 3, 2, 1, 12, 32, 1, y, NO_DEV) == FIR_ENODEV, "device lookup");
    expect(fir_cplx_resample_rows(x, 1, 16, h3, 3, 3, 2, 1, 12, 32, 1, y, -1) == FIR_ENODEV, "device -1");
    expect(fir_cplx_resample_last_launch(NULL, NULL) == FIR_OK, "last_launch with NULL outputs");

    /* the route query: reads the taps it is given and nothing else */
    {
        int bucket = -1;
        const uintptr_t X = (uintptr_t)1 << 30;
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 3, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_FAST && bucket == 1, "fast");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 2, 3, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_FAST && bucket == 2, "fast 2/3");
        expect(fir_cplx_resample_route(X, X + 4, 4, 4096, h3, 3, 16, 16, 15, 31, 1, 1, NULL) == FIR_CRESAMPLE_FAST, "fast, NULL bucket");
        expect(fir_cplx_resample_route(X + 4, X, 1, 4096, h3, 3, 3, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32 && bucket == 0, "x off 16");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 17, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32, "up 17");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 2, 17, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32, "decim 17");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 1, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32, "up 1");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 2, 1, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32, "decim 1");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 3, 2, 0, 12, 32, 0, &bucket) == FIR_CRESAMPLE_GENERIC32, "u8 stage");
        expect(fir_cplx_resample_route(X, X, 3, 4098, h3, 3, 3, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC32, "rows of 4k + 2");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 3, 2, 0, 12, 33, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "acc 33");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 3, 2, 0, 32, 32, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "frac 32");
        expect(fir_cplx_resample_route(X, X, 0, 4096, h3, 3, 3, 2, 0, 12, 32, 1, &bucket) == FIR_CRESAMPLE_NONE && bucket == 0, "empty");
        expect(fir_cplx_resample_route(X, X, 2, 1, h3, 3, 2, 16, 2, 12, 32, 1, &bucket) == FIR_CRESAMPLE_NONE && bucket == 0, "empty: phase");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 0, 2, 0, 12, 32, 1, &bucket) == -1 && said("up must be"), "refused");
        expect(fir_cplx_resample_route(X, X, 1, 4096, h3, 3, 3, 2, 2, 12, 32, 1, &bucket) == -1 && said("phase must be"), "refused: phase");
        expect(fir_cplx_resample_route(0, X, 1, 4096, h3, 3, 3, 2, 0, 12, 32, 1, &bucket) == -1 && said("NULL"), "refused: NULL x");
        /* every tap count 1..130 at every rate pair of 1..17, from a heap array of exactly that size */
        for (int L = 1; L <= 130; ++L) {
            int32_t* h = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)L);
            for (int k = 0; k < 2 * L; ++k) h[k] = (k % 7) - 3 + (k == 1);
            for (int U = 1; U <= 17; ++U)
                for (int D = 1; D <= 17; ++D) {
                    const int ph = (L + U) % D;
                    const int fast = U >= 2 && U <= 16 && D >= 2 && D <= 16 && L <= 128 && (L + U - 1) / U <= 32;
                    const int r = fir_cplx_resample_route(X, X, 2, 4096, h, L, U, D, ph, 12, 24, 1, &bucket);
                    expect(fast ? (r == FIR_CRESAMPLE_FAST && bucket == bucket_of(L, U, D, ph)) : (r == FIR_CRESAMPLE_GENERIC32 && bucket == 0),
                           "tap buckets");
                }
            h[2 * L - 1] = -32768;
            expect(fir_cplx_resample_route(X, X, 2, 4096, h, L, 3, 2, 1, 12, 24, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "a part of -32768");
            h[2 * L - 1] = INT32_MIN;
            h[0] = INT32_MAX;
            expect(fir_cplx_resample_route(X, X, 2, 4096, h, L, 3, 2, 1, 12, 64, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "int32 ends, narrow sum");
            free(h);
        }
        /* 128-bit sums: 2^16 + 9 complex taps of +-(2^31 - 1) */
        const int L = (1 << 16) + 9;
        int32_t* h = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)L);
        for (int k = 0; k < 2 * L; ++k) h[k] = (k & 1) ? -INT32_MAX : INT32_MAX;
        expect(fir_cplx_resample_route(X, X, 2, 150, h, L, 3, 2, 1, 30, 64, 1, &bucket) == FIR_CRESAMPLE_GENERIC128, "wide sums");
        expect(fir_cplx_resample_route(X, X, 2, 150, h, L, 3, 2, 1, 30, 63, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "acc 63");
        expect(fir_cplx_resample_route(X, X, 2, 150, h, (1 << 16) - 1, 3, 2, 1, 30, 64, 1, &bucket) == FIR_CRESAMPLE_GENERIC64, "below 2^63");
        free(h);
    }

    free(x);
    free(y);
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("cresample_check: ok\n");
    return 0;
}
