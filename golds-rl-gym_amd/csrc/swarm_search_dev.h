// The statements of the cross-entropy search over a Swarm rule's five real numbers (include/goldsrl_swarmsearch.h: 1 start,
// 2-4 candidates, incumbent and rows, 7 rank, 8 refit), shared by the translation units whose kernels run them (swarm_search.hip:
// one distribution for all envs, one workgroup; swarm_cemplan.hip: one distribution and one workgroup per env, at every decision of a
// planned episode) and the host's checks of the box.  One copy, so the planner's candidates, ranks and refits are the search's bits.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#include <string>

#include "common.h"

namespace grl {

constexpr int SEARCH_P = 5;                       // cancel, gain, off_x, off_y, radius
constexpr int SEARCH_MAX_C = 1024;                // one workgroup ranks a generation
__host__ __device__ constexpr int search_col(int k) { return k < 2 ? k : k + 1; }      // where parameter k stands in a six-number row

// what the statements read beside the distribution: the start, the spreads and the box, the ring and the anchor
struct SearchBox {
    double mean0[SEARCH_P], std0[SEARCH_P], floor[SEARCH_P], lo[SEARCH_P], hi[SEARCH_P];
    double ring[N_AGENTS][2];
    double anchor;
};

// the first operand wins a tie (goldsrl_swarmsearch.h); a select, never v_max/v_min, whose order of signed zeros is their own
__device__ __forceinline__ double first_max(double a, double b) { return a >= b ? a : b; }
__device__ __forceinline__ double first_min(double a, double b) { return a <= b ? a : b; }

// 1 start: parameter k of the start, clamped into the box
__device__ __forceinline__ double search_start(const SearchBox &B, int k) { return first_min(first_max(B.mean0[k], B.lo[k]), B.hi[k]); }

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

// 8 refit of parameter k over the K elites rows[order_s[0..K-1]] (six-number rows): two sequential chains in rank order
__device__ __forceinline__ void search_refit(const double *rows, const int *order_s, int K, int k, double floor, double &mean, double &std) {
    const int col = search_col(k);
    const double kk = (double)K;
    double m = 0.0;
    for (int i = 0; i < K; ++i) {
        const double p = rows[(size_t)order_s[i] * 6 + col];
        m = m + p;
    }
    m = m / kk;
    double s = 0.0;
    for (int i = 0; i < K; ++i) {
        const double p = rows[(size_t)order_s[i] * 6 + col];
        const double d = p - m;
        const double q = d * d;
        s = s + q;
    }
    const double v = s / kk;
    mean = m;
    std = first_max(sqrt(v), floor);
}

// 2-4: one candidate's six-number row, rule row and offsets.  incumbent: null, or the six numbers candidate 0 copies bit for bit
// (3; null for candidate 0 of generation 0: the mean itself).  z: the candidate's five normals (2; unread for candidate 0).
__device__ __forceinline__ void search_build(const SearchBox &B, const double *mean, const double *std, const double *z, bool is_incumbent,
                                             const double *incumbent, double *cand, double *rule, double *offsets) {
    double six[6];
    if (is_incumbent) {                           // 3 incumbent
        if (!incumbent) {
#pragma unroll
            for (int k = 0; k < SEARCH_P; ++k) six[search_col(k)] = mean[k];
            six[2] = B.anchor;
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) six[k] = incumbent[k];
        }
    } else {                                      // 2 candidates
#pragma unroll
        for (int k = 0; k < SEARCH_P; ++k) {
            double v = std[k] * z[k];
            v = mean[k] + v;
            v = first_max(v, B.lo[k]);
            v = first_min(v, B.hi[k]);
            six[search_col(k)] = v;
        }
        six[2] = B.anchor;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) cand[k] = six[k];
    rule[0] = six[0];                             // 4 rows
    rule[1] = six[1];
    rule[2] = six[2];
#pragma unroll
    for (int a = 0; a < N_AGENTS; ++a) {
        const double tx = six[5] * B.ring[a][0];
        const double ty = six[5] * B.ring[a][1];
        reinterpret_cast<double2 *>(offsets)[a] = make_double2(six[3] + tx, six[4] + ty);
    }
}

// The host's checks of the anchor and the counts, of the box and the ring.  fn: the C function's name, with which every message starts.
static int search_check_five(grl_handle *h, const char *fn, const char *noun, const double *v, bool non_negative) {
    for (int k = 0; k < SEARCH_P; ++k) {
        if (!std::isfinite(v[k])) return fail(h, GRL_E_INVALID, std::string(fn) + ": " + noun + "[" + std::to_string(k) + "] is not finite");
        if (non_negative && v[k] < 0) return fail(h, GRL_E_INVALID, std::string(fn) + ": " + noun + "[" + std::to_string(k) + "] is negative");
    }
    return GRL_OK;
}

static int search_check_counts(grl_handle *h, const char *fn, int anchor, int G, int C, int K) {
    const std::string f(fn);
    if (anchor != 0 && anchor != 1) return fail(h, GRL_E_INVALID, f + ": anchor must be 0 (centroid) or 1 (nearest locust)");
    if (G < 1) return fail(h, GRL_E_INVALID, f + ": G must be at least 1");
    if (C < 2 || C > SEARCH_MAX_C) return fail(h, GRL_E_INVALID, f + ": C must be in 2.." + std::to_string(SEARCH_MAX_C));
    if (K < 1 || K > C) return fail(h, GRL_E_INVALID, f + ": K must be in 1..C");
    return GRL_OK;
}

static int search_check_box(grl_handle *h, const char *fn, const double *mean0, const double *std0, const double *floor, const double *lo,
                            const double *hi, const double *ring) {
    const std::string f(fn);
    int rc;
    if ((rc = search_check_five(h, fn, "mean0", mean0, false)) || (rc = search_check_five(h, fn, "std0", std0, true)) ||
        (rc = search_check_five(h, fn, "floor", floor, true)) || (rc = search_check_five(h, fn, "lo", lo, false)) ||
        (rc = search_check_five(h, fn, "hi", hi, false)))
        return rc;
    for (int k = 0; k < SEARCH_P; ++k)
        if (lo[k] > hi[k]) return fail(h, GRL_E_INVALID, f + ": lo[" + std::to_string(k) + "] is above hi[" + std::to_string(k) + "]");
    for (int k = 0; k < N_AGENTS * 2; ++k)
        if (!std::isfinite(ring[k])) return fail(h, GRL_E_INVALID, f + ": ring[" + std::to_string(k / 2) + "] is not finite");
    return GRL_OK;
}

static void search_fill_box(SearchBox &B, int anchor, const double *mean0, const double *std0, const double *floor, const double *lo,
                            const double *hi, const double *ring) {
    for (int k = 0; k < SEARCH_P; ++k) { B.mean0[k] = mean0[k]; B.std0[k] = std0[k]; B.floor[k] = floor[k]; B.lo[k] = lo[k]; B.hi[k] = hi[k]; }
    for (int a = 0; a < N_AGENTS; ++a) { B.ring[a][0] = ring[a * 2]; B.ring[a][1] = ring[a * 2 + 1]; }
    B.anchor = (double)anchor;
}

}  // namespace grl
