// What is Ticker's own in the cross-entropy search over the six numbers of a Ticker rule (include/goldsrl_tickersearch.h:
// 2 candidates, 3 row, 4 incumbent): candidates that end as float32 rows which stay a rule of grl_ticker_sweep.  The clamp, the draw,
// the fit's sum (6), the rank (7) and the refit (8) are search_dev.h's, which the Swarm searches share; nothing of Swarm is included.
// The candidate and row statements are __host__ __device__: the host builds generation 0's table with them (IEEE float64 operations,
// rint and the float casts give the same bits on both sides), the update kernel every later one.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <string.h>

#include "search_dev.h"

namespace grl {

constexpr int TSEARCH_P = 6;                      // up0, up1, dn0, dn1, band, lookback: a row of grl_ticker_sweep

// what the statements read beside the distribution: the spreads' floors and the box (the start is spent on the host, in generation 0)
struct TickerSearchBox {
    double floor[TSEARCH_P], lo[TSEARCH_P], hi[TSEARCH_P];
};

// the next float32 towards zero of a positive finite f
__host__ __device__ __forceinline__ float ticker_search_below(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    b -= 1u;
    memcpy(&f, &b, 4);
    return f;
}

// 3 row: six float64 numbers inside the box as the float32 row that is played.  The casts round to nearest, so a pair of weights
// may sum above 1 where the float64 numbers did not, and 1 - f_a cast to float32 may again; one step down always ends it.
__host__ __device__ __forceinline__ void ticker_search_row(const double *v, float *f) {
#pragma unroll
    for (int k = 0; k < 5; ++k) f[k] = (float)v[k];
    f[5] = (float)rint(v[5]);
#pragma unroll
    for (int a = 0; a < 4; a += 2) {
        const int b = a + 1;
        double s = (double)f[a] + (double)f[b];
        if (s > 1.0) {
            const double t = 1.0 - (double)f[a];
            f[b] = (float)t;
            s = (double)f[a] + (double)f[b];
            if (s > 1.0) f[b] = ticker_search_below(f[b]);
        }
    }
}

// 2-4: row c of a generation's table.  incumbent: null, or the row candidate 0 copies bit for bit (4; null in generation 0, where
// candidate 0 is statement 3 of the mean).  z: the candidate's six normals (unread for candidate 0).
__host__ __device__ __forceinline__ void ticker_search_build(const TickerSearchBox &B, const double *mean, const double *std, const double *z,
                                                             bool is_incumbent, const float *incumbent, float *row) {
    float f[TSEARCH_P];
    if (is_incumbent && incumbent) {
#pragma unroll
        for (int k = 0; k < TSEARCH_P; ++k) f[k] = incumbent[k];
    } else {
        double v[TSEARCH_P];
#pragma unroll
        for (int k = 0; k < TSEARCH_P; ++k) v[k] = is_incumbent ? mean[k] : search_draw(mean[k], std[k], z[k], B.lo[k], B.hi[k]);
        ticker_search_row(v, f);
    }
#pragma unroll
    for (int k = 0; k < TSEARCH_P; ++k) row[k] = f[k];
}

}  // namespace grl
