// What is Swarm's own in the cross-entropy search over a Swarm rule's five real numbers (include/goldsrl_swarmsearch.h: 1 start,
// 2-4 candidates, incumbent and rows): where the five stand in a six-number row, the box, the ring and the anchor, the candidate's
// rule row and offsets, and the host's checks of them.  The clamp, the draw, the rank (7) and the refit (8) are search_dev.h's, which
// the Ticker search shares.  Included by the translation units whose kernels run the statements (swarm_search.hip: one distribution
// for all envs, one workgroup; swarm_cemplan.hip: one distribution and one workgroup per env, at every decision of a planned
// episode).  One copy, so the planner's candidates, ranks and refits are the search's bits.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include "search_dev.h"

namespace grl {

constexpr int SEARCH_P = 5;                       // cancel, gain, off_x, off_y, radius
__host__ __device__ constexpr int search_col(int k) { return k < 2 ? k : k + 1; }      // where parameter k stands in a six-number row

// what the statements read beside the distribution: the start, the spreads and the box, the ring and the anchor
struct SearchBox {
    double mean0[SEARCH_P], std0[SEARCH_P], floor[SEARCH_P], lo[SEARCH_P], hi[SEARCH_P];
    double ring[N_AGENTS][2];
    double anchor;
};

// 1 start: parameter k of the start, clamped into the box
__device__ __forceinline__ double search_start(const SearchBox &B, int k) { return search_clamp(B.mean0[k], B.lo[k], B.hi[k]); }

// 8 refit of parameter k: search_dev.h's two chains, over six-number rows.  (Through this call the two update kernels compile to the
// instructions they had; with search_refit_rows written out at the call sites the compiler swapped two of them.)
__device__ __forceinline__ void search_refit(const double *rows, const int *order_s, int K, int k, double floor, double &mean, double &std) {
    search_refit_rows<double>(rows, 6, order_s, K, search_col(k), floor, mean, std);
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
        for (int k = 0; k < SEARCH_P; ++k) six[search_col(k)] = search_draw(mean[k], std[k], z[k], B.lo[k], B.hi[k]);
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

// The host's checks of the anchor, the box and the ring.  fn: the C function's name, with which every message starts.
static int search_check_anchor(grl_handle *h, const char *fn, int anchor) {
    if (anchor != 0 && anchor != 1) return fail(h, GRL_E_INVALID, std::string(fn) + ": anchor must be 0 (centroid) or 1 (nearest locust)");
    return GRL_OK;
}

static int search_check_box(grl_handle *h, const char *fn, const double *mean0, const double *std0, const double *floor, const double *lo,
                            const double *hi, const double *ring) {
    const std::string f(fn);
    int rc;
    const struct { const char *noun; const double *v; bool non_negative; } five[] = {
        {"mean0", mean0, false}, {"std0", std0, true}, {"floor", floor, true}, {"lo", lo, false}, {"hi", hi, false}};
    for (const auto &v : five)
        if ((rc = search_check_vector(h, fn, v.noun, v.v, SEARCH_P, nullptr, v.non_negative))) return rc;
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
