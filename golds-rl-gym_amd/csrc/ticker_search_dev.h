// The statements of the cross-entropy search over the six numbers of a Ticker rule (include/goldsrl_tickersearch.h: 1 start,
// 2 candidates, 3 row, 4 incumbent, 8 refit) that are not the Swarm search's: candidates that end as float32 rows which stay a rule
// of grl_ticker_sweep, and a refit over such rows.  first_max, first_min and the rank (7) are swarm_search_dev.h's, unchanged.
// The candidate and row statements are __host__ __device__: the host builds generation 0's table with them (IEEE float64 operations,
// rint and the float casts give the same bits on both sides), the update kernel every later one.  The refit knows nothing of the
// Ticker rule: rows of any element type and width, so a two-number TradeAR1 search can call it.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "swarm_search_dev.h"

namespace grl {

constexpr int TSEARCH_P = 6;                      // up0, up1, dn0, dn1, band, lookback: a row of grl_ticker_sweep

// what the statements read beside the distribution: the spreads' floors and the box (the start is spent on the host, in generation 0)
struct TickerSearchBox {
    double floor[TSEARCH_P], lo[TSEARCH_P], hi[TSEARCH_P];
};

// 1 start / 2 candidates: the clamp into the box, the first operand winning a tie (first_max and first_min, for both sides)
__host__ __device__ __forceinline__ double ticker_search_clamp(double v, double lo, double hi) {
    v = v >= lo ? v : lo;
    v = v <= hi ? v : hi;
    return v;
}

// 2 candidates: one number of one candidate
__host__ __device__ __forceinline__ double ticker_search_draw(double mean, double std, double z, double lo, double hi) {
    double v = std * z;
    v = mean + v;
    return ticker_search_clamp(v, lo, hi);
}

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
        for (int k = 0; k < TSEARCH_P; ++k) v[k] = is_incumbent ? mean[k] : ticker_search_draw(mean[k], std[k], z[k], B.lo[k], B.hi[k]);
        ticker_search_row(v, f);
    }
#pragma unroll
    for (int k = 0; k < TSEARCH_P; ++k) row[k] = f[k];
}

// 6 fit, the sum: s = 0.0; s = s + scores[c][e] for e in index order, for the (C, E) scores of one generation.  Called by EVERY lane
// of the 1 024-lane workgroup (two barriers per tile); lane c < C gets its candidate's sum, the other lanes 0.  A lane that read its
// own row would load 8 bytes at a stride of E * 8 from its neighbours' -- measured at 8 192 envs x 64 candidates that way, the update
// kernel was a sixth of the whole call.  So the workgroup stages the scores through LDS in tiles of all C rows x TE envs: the loads
// run along the rows (TE consecutive doubles per row, consecutive lanes on consecutive envs), the next tile's are in flight in
// registers while lane c adds the current tile's row c from LDS, left to right.  One accumulator per candidate, tiles in env order:
// the add order is the statement's.  The LDS row stride is odd, so the C lanes of the add read different banks.
constexpr int SEARCH_TILE = 4096;                               // scores staged per tile: C * TE <= SEARCH_TILE, TE >= 4 at C = 1 024
constexpr int SEARCH_TILE_LDS = SEARCH_TILE + SEARCH_MAX_C;     // doubles: C * (TE | 1) <= C * TE + C
constexpr int SEARCH_TILE_REGS = SEARCH_TILE / SEARCH_MAX_C;    // tile elements per lane

__device__ __forceinline__ double search_fit_sum(const double *__restrict__ scores, int C, int E, int c, double *tile_s) {
    const int TE = max(1, min(E, SEARCH_TILE / C)), RS = TE | 1, n_tile = C * TE;
    int row[SEARCH_TILE_REGS], col[SEARCH_TILE_REGS];
    double r[SEARCH_TILE_REGS];
#pragma unroll
    for (int u = 0; u < SEARCH_TILE_REGS; ++u) {
        const int i = c + u * SEARCH_MAX_C;                     // c is the lane: threadIdx.x
        row[u] = i / TE;
        col[u] = i - row[u] * TE;
        if (i >= n_tile) row[u] = -1;
        r[u] = (row[u] >= 0 && col[u] < E) ? scores[(size_t)row[u] * E + col[u]] : 0.0;
    }
    double s = 0.0;
    for (int e0 = 0; e0 < E; e0 += TE) {
#pragma unroll
        for (int u = 0; u < SEARCH_TILE_REGS; ++u)
            if (row[u] >= 0) tile_s[row[u] * RS + col[u]] = r[u];
        __syncthreads();
        const int e1 = e0 + TE;
        if (e1 < E) {
#pragma unroll
            for (int u = 0; u < SEARCH_TILE_REGS; ++u)
                r[u] = (row[u] >= 0 && e1 + col[u] < E) ? scores[(size_t)row[u] * E + e1 + col[u]] : 0.0;
        }
        if (c < C) {
            const int n = min(TE, E - e0);
            const double *mine = tile_s + c * RS;
            for (int j = 0; j < n; ++j) s = s + mine[j];
        }
        __syncthreads();
    }
    return c < C ? s : 0.0;
}

// 8 refit of column `col` over the K elites rows[order_s[0..K-1]] (rows of `width` numbers of type T, widened to float64): two
// sequential chains in rank order
template <typename T>
__device__ __forceinline__ void search_refit_rows(const T *rows, int width, const int *order_s, int K, int col, double floor, double &mean,
                                                  double &std) {
    const double kk = (double)K;
    double m = 0.0;
    for (int i = 0; i < K; ++i) {
        const double p = (double)rows[(size_t)order_s[i] * width + col];
        m = m + p;
    }
    m = m / kk;
    double s = 0.0;
    for (int i = 0; i < K; ++i) {
        const double p = (double)rows[(size_t)order_s[i] * width + col];
        const double d = p - m;
        const double q = d * d;
        s = s + q;
    }
    const double v = s / kk;
    mean = m;
    std = first_max(sqrt(v), floor);
}

}  // namespace grl
