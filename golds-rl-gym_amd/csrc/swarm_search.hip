// Cross-entropy search over the five real numbers of a Swarm feedback rule, all G generations enqueued in ONE call (C ABI and the
// scheme, statement by statement: include/goldsrl_swarmsearch.h).  Per generation two kernels, all on the handle's stream; nothing is
// read back between them.
//   evaluate  swarm_plan_kernel<MATH, false> (swarm_plan_dev.h), the planner's lookahead: one (env, candidate) pair per 80 lanes, one
//             8-byte score per pair at ((env * G + g) * C + c), the generation's table read from device memory.  horizon = max_steps
//             and a clock that stays at zero make it grl_swarm_rules(max_steps) of the table.  No copy of the step loop here.
//   update    one workgroup: the fit of every candidate (a sequential sum over the envs), its rank, the refit of mean and std over
//             the elites, and the next generation's candidates, rule rows and offsets.  Launched once before generation 0, where it
//             only clamps the start and builds the table, and once after the last, where it builds none: G + 1 launches, so the
//             candidate statements exist in this one form.
// The handle's state is read only: positions, noise rows and elapsed are read, nothing of it is written.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_plan_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmsearch.h"

namespace grl {

constexpr int SEARCH_P = 5;                       // cancel, gain, off_x, off_y, radius
constexpr int SEARCH_MAX_C = 1024;                // one workgroup ranks a generation
__host__ __device__ constexpr int search_col(int k) { return k < 2 ? k : k + 1; }      // where parameter k stands in a six-number row

struct SearchParams {
    const double *z;                              // (G, C, 5): the host's normals
    const double *scores;                         // (E, G, C)
    double *cand, *rules, *offsets;               // (G, C, 6) (G, C, 3) (G, C, 10, 2)
    double *fit;                                  // (G, C)
    int32_t *order;                               // (G, C)
    double *mean, *std;                           // (G + 1, 5) each
    double mean0[SEARCH_P], std0[SEARCH_P], floor[SEARCH_P], lo[SEARCH_P], hi[SEARCH_P];
    double ring[N_AGENTS][2];
    double anchor;
    int E, G, C, K, g;                            // g: the generation whose table this launch builds (G: none)
};

// the first operand wins a tie (goldsrl_swarmsearch.h); a select, never v_max/v_min, whose order of signed zeros is their own
__device__ __forceinline__ double first_max(double a, double b) { return a >= b ? a : b; }
__device__ __forceinline__ double first_min(double a, double b) { return a <= b ? a : b; }

// One workgroup of 1 024 lanes, lane c owning candidate c; lanes past C only keep the barriers (every lane reaches all of them: no
// early return).  The chains are short and latency bound (E loads per lane for the fit, C LDS reads for the rank, 2 K loads on five
// lanes for the refit), and there is one workgroup, so neither occupancy nor bandwidth is the matter; the kernel exists to keep the
// generations on the device.
// Launch bounds 1 024 (the most a workgroup holds: 16 waves of 64).  Compiled (hipcc -O3, gfx950): 54 VGPRs, 12 376 bytes of LDS
// (fit 8 192, order 4 096, mean and std 80, 8 of alignment), 0 bytes of scratch.  Measured: profiles/swarm_search_times.json.
__global__ __launch_bounds__(SEARCH_MAX_C) void swarm_search_update_kernel(SearchParams P) {
    __shared__ double fit_s[SEARCH_MAX_C];
    __shared__ int order_s[SEARCH_MAX_C];
    __shared__ double mean_s[SEARCH_P], std_s[SEARCH_P];
    const int c = threadIdx.x, C = P.C, g = P.g;
    const bool mine = c < C;

    if (g == 0) {
        if (c < SEARCH_P) {                       // 1 start
            const double m = first_min(first_max(P.mean0[c], P.lo[c]), P.hi[c]);
            mean_s[c] = m;
            std_s[c] = P.std0[c];
            P.mean[c] = m;
            P.std[c] = P.std0[c];
        }
    } else {
        const size_t prev = (size_t)(g - 1) * C;
        double f = 0.0;
        if (mine) {                               // 6 fit
            double s = 0.0;
            for (int e = 0; e < P.E; ++e) s = s + P.scores[((size_t)e * P.G + (g - 1)) * C + c];
            f = s / (double)P.E;
            P.fit[prev + c] = f;
            fit_s[c] = f;
            order_s[c] = c;                       // fits that are no total order (a NaN) leave ranks unclaimed: those slots stay indices
        }
        __syncthreads();
        if (mine) {                               // 7 rank: how many candidates stand before this one
            int rank = 0;
            for (int i = 0; i < C; ++i) {
                const double o = fit_s[i];
                rank += (o > f || (o == f && i < c)) ? 1 : 0;
            }
            order_s[rank] = c;                    // rank < C: at most the C - 1 others count
            P.order[prev + rank] = c;
        }
        __syncthreads();
        if (c < SEARCH_P) {                       // 8 refit: two sequential chains in rank order
            const int col = search_col(c);
            const double kk = (double)P.K;
            double m = 0.0;
            for (int i = 0; i < P.K; ++i) {
                const double p = P.cand[(prev + order_s[i]) * 6 + col];
                m = m + p;
            }
            m = m / kk;
            double s = 0.0;
            for (int i = 0; i < P.K; ++i) {
                const double p = P.cand[(prev + order_s[i]) * 6 + col];
                const double d = p - m;
                const double q = d * d;
                s = s + q;
            }
            const double v = s / kk;
            const double sd = first_max(sqrt(v), P.floor[c]);
            mean_s[c] = m;
            std_s[c] = sd;
            P.mean[(size_t)g * SEARCH_P + c] = m;
            P.std[(size_t)g * SEARCH_P + c] = sd;
        }
    }
    __syncthreads();

    if (g < P.G && mine) {                        // 2-4: generation g's table
        const size_t row = (size_t)g * C + c;
        double six[6];
        if (c == 0) {                             // 3 incumbent
            if (g == 0) {
#pragma unroll
                for (int k = 0; k < SEARCH_P; ++k) six[search_col(k)] = mean_s[k];
                six[2] = P.anchor;
            } else {
                const double *best = P.cand + ((size_t)(g - 1) * C + order_s[0]) * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) six[k] = best[k];
            }
        } else {                                  // 2 candidates
            const double *z = P.z + row * SEARCH_P;
#pragma unroll
            for (int k = 0; k < SEARCH_P; ++k) {
                double v = std_s[k] * z[k];
                v = mean_s[k] + v;
                v = first_max(v, P.lo[k]);
                v = first_min(v, P.hi[k]);
                six[search_col(k)] = v;
            }
            six[2] = P.anchor;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) P.cand[row * 6 + k] = six[k];
        P.rules[row * 3 + 0] = six[0];            // 4 rows
        P.rules[row * 3 + 1] = six[1];
        P.rules[row * 3 + 2] = six[2];
#pragma unroll
        for (int a = 0; a < N_AGENTS; ++a) {
            const double tx = six[5] * P.ring[a][0];
            const double ty = six[5] * P.ring[a][1];
            reinterpret_cast<double2 *>(P.offsets)[row * N_AGENTS + a] = make_double2(six[3] + tx, six[4] + ty);
        }
    }
}

static int search_check_five(grl_handle *h, const char *noun, const double *v, bool non_negative) {
    for (int k = 0; k < SEARCH_P; ++k) {
        if (!std::isfinite(v[k])) return fail(h, GRL_E_INVALID, std::string("grl_swarm_search: ") + noun + "[" + std::to_string(k) + "] is not finite");
        if (non_negative && v[k] < 0) return fail(h, GRL_E_INVALID, std::string("grl_swarm_search: ") + noun + "[" + std::to_string(k) + "] is negative");
    }
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_swarm_search(grl_handle *h, int32_t anchor, const double *mean0, const double *std0, const double *floor, const double *lo,
                     const double *hi, const double *ring, const double *normals, int32_t G, int32_t C, int32_t K, int32_t max_steps) {
    const char *fn = "grl_swarm_search";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", mean0 && std0 && floor && lo && hi && ring && normals))) return rc;
    if (anchor != 0 && anchor != 1) return fail(h, GRL_E_INVALID, "grl_swarm_search: anchor must be 0 (centroid) or 1 (nearest locust)");
    if (G < 1) return fail(h, GRL_E_INVALID, "grl_swarm_search: G must be at least 1");
    if (C < 2 || C > SEARCH_MAX_C) return fail(h, GRL_E_INVALID, "grl_swarm_search: C must be in 2.." + std::to_string(SEARCH_MAX_C));
    if (K < 1 || K > C) return fail(h, GRL_E_INVALID, "grl_swarm_search: K must be in 1..C");
    if ((rc = episode_check_steps(h, fn, max_steps)) || (rc = search_check_five(h, "mean0", mean0, false)) ||
        (rc = search_check_five(h, "std0", std0, true)) || (rc = search_check_five(h, "floor", floor, true)) ||
        (rc = search_check_five(h, "lo", lo, false)) || (rc = search_check_five(h, "hi", hi, false)))
        return rc;
    for (int k = 0; k < SEARCH_P; ++k)
        if (lo[k] > hi[k]) return fail(h, GRL_E_INVALID, "grl_swarm_search: lo[" + std::to_string(k) + "] is above hi[" + std::to_string(k) + "]");
    for (int k = 0; k < N_AGENTS * 2; ++k)
        if (!std::isfinite(ring[k])) return fail(h, GRL_E_INVALID, "grl_swarm_search: ring[" + std::to_string(k / 2) + "] is not finite");
    const size_t E = (size_t)h->E, gc = (size_t)G * C, scores = E * gc;
    const size_t largest = std::max(scores, gc * N_AGENTS * 2);
    if (largest > (size_t)INT32_MAX)
        return fail(h, GRL_E_INVALID, "grl_swarm_search: an output of " + std::to_string(largest) +
                                          " elements does not fit in int32 (fewer envs, generations or candidates per call)");
    for (size_t i = 0; i < gc * SEARCH_P; ++i)
        if (!std::isfinite(normals[i])) return fail(h, GRL_E_INVALID, "grl_swarm_search: normals[" + std::to_string(i) + "] is not finite");
    if ((rc = episode_check_idle(h, fn))) return rc;
    hipSetDevice(h->cfg.device_id);
    SwarmSearchState &w = h->ssr;
    w.G = 0;
    if ((rc = episode_reserve(h, w.cap_gc, gc, {buf(w.normals, SEARCH_P), buf(w.cand, 6), buf(w.rules, 3), buf(w.offsets, N_AGENTS * 2), buf(w.fit), buf(w.order)})) ||
        (rc = episode_reserve(h, w.cap_scores, scores, {buf(w.scores)})) ||
        (rc = episode_reserve(h, w.cap_gen, (size_t)G + 1, {buf(w.mean, SEARCH_P), buf(w.std, SEARCH_P)})) ||
        (rc = episode_reserve(h, w.cap_envs, E, {buf(w.length), buf(w.finished)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.normals, normals, gc * SEARCH_P * 8, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.length, 0, E * 4, h->stream));           // the lookahead's clock: every generation starts at the handle's state
    GRL_HIP(h, hipMemsetAsync(w.finished, 0, E, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.scores, 0, scores * 8, h->stream));

    SearchParams S{};
    S.z = w.normals; S.scores = w.scores; S.cand = w.cand; S.rules = w.rules; S.offsets = w.offsets;
    S.fit = w.fit; S.order = w.order; S.mean = w.mean; S.std = w.std;
    for (int k = 0; k < SEARCH_P; ++k) { S.mean0[k] = mean0[k]; S.std0[k] = std0[k]; S.floor[k] = floor[k]; S.lo[k] = lo[k]; S.hi[k] = hi[k]; }
    for (int a = 0; a < N_AGENTS; ++a) { S.ring[a][0] = ring[a * 2]; S.ring[a][1] = ring[a * 2 + 1]; }
    S.anchor = (double)anchor; S.E = h->E; S.G = G; S.C = C; S.K = K;

    PlanParams P{};                               // the planner's lookahead: D decisions are the G generations, the table generation g's
    swarm_start_state(h, P);
    P.length = w.length; P.finished = w.finished; P.scores = w.scores;
    P.E = h->E; P.n_rules = C; P.horizon = max_steps; P.replan = max_steps; P.max_steps = max_steps;
    P.limit = h->cfg.max_episode_steps; P.trace_env = -1; P.D = G;
    const dim3 look((unsigned)((E * C + SWARM_EPB - 1) / SWARM_EPB)), block(SWARM_TPB);
    rc = episode_launch(h, [&] {                  // the math mode selects block_step, never the rule's or the search's statements
        swarm_math_dispatch(h, [&](auto M) {
            for (int g = 0; g <= G; ++g) {
                S.g = g;
                hipLaunchKernelGGL(swarm_search_update_kernel, dim3(1), dim3(SEARCH_MAX_C), 0, h->stream, S);
                if (g == G) break;
                P.d = g;
                P.rules = w.rules + (size_t)g * C * 3;
                P.offsets = w.offsets + (size_t)g * C * N_AGENTS * 2;
                hipLaunchKernelGGL((swarm_plan_kernel<decltype(M)::value, false>), look, block, 0, h->stream, P);
            }
        });
    });
    if (rc) return rc;
    w.G = G; w.C = C;
    return GRL_OK;
}

int grl_swarm_search_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SwarmSearchState &w = h->ssr;
    const size_t E = (size_t)h->E, gc = (size_t)w.G * w.C, gen = (size_t)w.G + 1;
    const EpisodeOut outs[] = {
        {"candidates", w.cand, gc * 6 * 8}, {"offsets", w.offsets, gc * N_AGENTS * 2 * 8}, {"scores", w.scores, E * gc * 8},
        {"fit", w.fit, gc * 8}, {"order", w.order, gc * 4}, {"mean", w.mean, gen * SEARCH_P * 8}, {"std", w.std, gen * SEARCH_P * 8}};
    return episode_read(h, "grl_swarm_search_read", GRL_ENV_SWARM, "Swarm", w.G != 0, "grl_swarm_search", outs, nullptr, which, host, bytes);
}

}  // extern "C"
