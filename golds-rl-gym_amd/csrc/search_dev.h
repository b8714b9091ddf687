// The statements of a cross-entropy search that know nothing of the env whose rule is searched (the numbering is that of
// include/goldsrl_swarmsearch.h and include/goldsrl_tickersearch.h: 1 and 2 the clamp and the draw, 6 the fit's sum, 7 rank, 8 refit),
// and the host's checks of what every such search takes: the counts, the per-parameter vectors, the normals, the output sizes.  One
// copy for swarm_search.hip, swarm_cemplan.hip, ticker_search.hip and trade_search.hip (through their *_search_dev.h, which add
// their rule's row and box), so a tie rule, a message or the refit is changed in one place and the searches cannot drift apart.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "common.h"

namespace grl {

constexpr int SEARCH_MAX_C = 1024;                // one workgroup ranks a generation

// the first operand wins a tie (goldsrl_swarmsearch.h); a select, never v_max/v_min, whose order of signed zeros is their own.
// __host__ __device__: the Ticker search builds generation 0 on the host with the same statements.
__host__ __device__ __forceinline__ double first_max(double a, double b) { return a >= b ? a : b; }
__host__ __device__ __forceinline__ double first_min(double a, double b) { return a <= b ? a : b; }

// 1 start / 2 candidates: the clamp into the box
__host__ __device__ __forceinline__ double search_clamp(double v, double lo, double hi) { return first_min(first_max(v, lo), hi); }

// 2 candidates: one number of one candidate
__host__ __device__ __forceinline__ double search_draw(double mean, double std, double z, double lo, double hi) {
    double v = std * z;
    v = mean + v;
    return search_clamp(v, lo, hi);
}

// 6 fit, the sum: s = 0.0; s = s + scores[c][e] for e in index order, for the (C, E) scores of one generation.  Called by EVERY lane
// of the 1 024-lane workgroup (two barriers per tile); lane c < C gets its candidate's sum, the other lanes 0.  A lane that read its
// own row would load 8 bytes at a stride of E * 8 from its neighbours' -- measured at 8 192 envs x 64 candidates that way, the update
// kernel was a sixth of the whole call.  So the workgroup stages the scores through LDS in tiles of all C rows x TE envs: the loads
// run along the rows (TE consecutive doubles per row, consecutive lanes on consecutive envs), the next tile's are in flight in
// registers while lane c adds the current tile's row c from LDS, left to right.  One accumulator per candidate, tiles in env order:
// the add order is the statement's.  The LDS row stride is odd, so the C lanes of the add read different banks.
// (The Swarm kernels' scores are laid out (E, G, C) and per env: they keep their own loops.)
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

// 7 rank: how many candidates stand before this one.  Called by EVERY lane of the workgroup (two barriers inside); lane c < C owns
// candidate c with fit f.  Leaves fit_s[c] = f and order_s[rank] = c in LDS for the lanes behind the second barrier, and writes
// order_out[rank] = c.  Fits that are no total order (a NaN) leave ranks unclaimed: those slots of order_s stay indices.
__device__ __forceinline__ void search_rank(double *fit_s, int *order_s, int c, int C, double f, int32_t *order_out) {
    const bool mine = c < C;
    if (mine) {
        fit_s[c] = f;
        order_s[c] = c;
    }
    __syncthreads();
    if (mine) {
        int rank = 0;
        for (int i = 0; i < C; ++i) {
            const double o = fit_s[i];
            rank += (o > f || (o == f && i < c)) ? 1 : 0;
        }
        order_s[rank] = c;                        // rank < C: at most the C - 1 others count
        order_out[rank] = c;
    }
    __syncthreads();
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

// The host's checks.  fn: the C function's name, with which every message starts.
static int search_check_counts(grl_handle *h, const char *fn, int G, int C, int K) {
    const std::string f(fn);
    if (G < 1) return fail(h, GRL_E_INVALID, f + ": G must be at least 1");
    if (C < 2 || C > SEARCH_MAX_C) return fail(h, GRL_E_INVALID, f + ": C must be in 2.." + std::to_string(SEARCH_MAX_C));
    if (K < 1 || K > C) return fail(h, GRL_E_INVALID, f + ": K must be in 1..C");
    return GRL_OK;
}

// one number per parameter: finite, and not negative where that is asked.  names: null, or the P parameters' names for the message
static int search_check_vector(grl_handle *h, const char *fn, const char *noun, const double *v, int P, const char *const *names, bool non_negative) {
    for (int k = 0; k < P; ++k) {
        const std::string at = std::string(fn) + ": " + noun + "[" + std::to_string(k) + "]" + (names ? std::string(" (") + names[k] + ")" : std::string());
        if (!std::isfinite(v[k])) return fail(h, GRL_E_INVALID, at + " is not finite");
        if (non_negative && v[k] < 0) return fail(h, GRL_E_INVALID, at + " is negative");
    }
    return GRL_OK;
}

static int search_check_normals(grl_handle *h, const char *fn, const double *normals, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(normals[i])) return fail(h, GRL_E_INVALID, std::string(fn) + ": normals[" + std::to_string(i) + "] is not finite");
    return GRL_OK;
}

// no output may hold more elements than an int32 counts.  fewer: what the caller can take less of, the end of the sentence
static int search_check_int32(grl_handle *h, const char *fn, size_t largest, const char *fewer) {
    if (largest > (size_t)INT32_MAX)
        return fail(h, GRL_E_INVALID, std::string(fn) + ": an output of " + std::to_string(largest) + " elements does not fit in int32 (" + fewer + ")");
    return GRL_OK;
}

}  // namespace grl
