// What is TradeAR1's own in the cross-entropy search over the four numbers of its rule (include/goldsrl_tradesearch.h: 3 row,
// 4 incumbent): candidates that end as float32 rows (gain_buy, gain_sell, bias, ref), every finite one a rule.  The clamp, the draw,
// the fit's sum (6), the rank (7) and the refit (8) are search_dev.h's, which the Swarm and Ticker searches share.
// trade_search_build is __host__ __device__: the host builds generation 0's table with it (IEEE float64 operations and the float
// casts give the same bits on both sides), the update kernel every later one.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include "search_dev.h"

namespace grl {

constexpr int TRSEARCH_P = 4;                     // gain_buy, gain_sell, bias, ref

// what the statements read beside the distribution: the spreads' floors and the box (the start is spent on the host, in generation 0)
struct TradeSearchBox {
    double floor[TRSEARCH_P], lo[TRSEARCH_P], hi[TRSEARCH_P];
};

// 2-4: row c of a generation's table.  incumbent: null, or the row candidate 0 copies bit for bit (4; null in generation 0, where
// candidate 0 is statement 3 of the mean).  z: the candidate's four normals (unread for candidate 0).
__host__ __device__ __forceinline__ void trade_search_build(const TradeSearchBox &B, const double *mean, const double *std, const double *z,
                                                            bool is_incumbent, const float *incumbent, float *row) {
    float f[TRSEARCH_P];
    if (is_incumbent && incumbent) {
#pragma unroll
        for (int k = 0; k < TRSEARCH_P; ++k) f[k] = incumbent[k];
    } else {
#pragma unroll
        for (int k = 0; k < TRSEARCH_P; ++k) {
            const double v = is_incumbent ? mean[k] : search_draw(mean[k], std[k], z[k], B.lo[k], B.hi[k]);
            f[k] = (float)v;                      // 3 row
        }
    }
#pragma unroll
    for (int k = 0; k < TRSEARCH_P; ++k) row[k] = f[k];
}

}  // namespace grl
