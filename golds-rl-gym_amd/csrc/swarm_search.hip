// Cross-entropy search over the five real numbers of a Swarm feedback rule, all G generations enqueued in ONE call (C ABI and the
// scheme, statement by statement: include/goldsrl_swarmsearch.h).  Per generation two kernels, all on the handle's stream; nothing is
// read back between them.
//   evaluate  swarm_plan_kernel<MATH, false> (swarm_plan_dev.h), the planner's lookahead: one (env, candidate) pair per 80 lanes, one
//             8-byte score per pair at ((env * G + g) * C + c), the generation's table read from device memory.  horizon = max_steps
//             and a clock that stays at zero make it grl_swarm_rules(max_steps) of the table.  No copy of the step loop here.
//   update    one workgroup: the fit of every candidate (a sequential sum over the envs), its rank, the refit of mean and std over
//             the elites, and the next generation's candidates, rule rows and offsets.  Launched once before generation 0, where it
//             only clamps the start and builds the table, and once after the last, where it builds none: G + 1 launches.  The
//             statements themselves are device functions: the clamp, the draw, the rank and the refit of search_dev.h (the Ticker
//             search's too), the Swarm row of swarm_search_dev.h, which the per-env planner (swarm_cemplan.hip) calls too: they
//             exist in that one form.
// The handle's state is read only: positions, noise rows and elapsed are read, nothing of it is written.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_plan_dev.h"
#include "swarm_search_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmsearch.h"

namespace grl {

struct SearchParams {
    const double *z;                              // (G, C, 5): the host's normals
    const double *scores;                         // (E, G, C)
    double *cand, *rules, *offsets;               // (G, C, 6) (G, C, 3) (G, C, 10, 2)
    double *fit;                                  // (G, C)
    int32_t *order;                               // (G, C)
    double *mean, *std;                           // (G + 1, 5) each
    SearchBox B;
    int E, G, C, K, g;                            // g: the generation whose table this launch builds (G: none)
};

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
            const double m = search_start(P.B, c);
            mean_s[c] = m;
            std_s[c] = P.B.std0[c];
            P.mean[c] = m;
            P.std[c] = P.B.std0[c];
        }
    } else {
        const size_t prev = (size_t)(g - 1) * C;
        double f = 0.0;
        if (mine) {                               // 6 fit
            double s = 0.0;
            for (int e = 0; e < P.E; ++e) s = s + P.scores[((size_t)e * P.G + (g - 1)) * C + c];
            f = s / (double)P.E;
            P.fit[prev + c] = f;
        }
        search_rank(fit_s, order_s, c, C, f, P.order + prev);                  // 7 rank
        if (c < SEARCH_P) {                       // 8 refit
            double m, sd;
            search_refit(P.cand + prev * 6, order_s, P.K, c, P.B.floor[c], m, sd);
            mean_s[c] = m;
            std_s[c] = sd;
            P.mean[(size_t)g * SEARCH_P + c] = m;
            P.std[(size_t)g * SEARCH_P + c] = sd;
        }
    }
    __syncthreads();

    if (g < P.G && mine) {                        // 2-4: generation g's table
        const size_t row = (size_t)g * C + c;
        search_build(P.B, mean_s, std_s, P.z + row * SEARCH_P, c == 0, g == 0 ? nullptr : P.cand + ((size_t)(g - 1) * C + order_s[0]) * 6,
                     P.cand + row * 6, P.rules + row * 3, P.offsets + row * N_AGENTS * 2);
    }
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_swarm_search(grl_handle *h, int32_t anchor, const double *mean0, const double *std0, const double *floor, const double *lo,
                     const double *hi, const double *ring, const double *normals, int32_t G, int32_t C, int32_t K, int32_t max_steps) {
    const char *fn = "grl_swarm_search";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", mean0 && std0 && floor && lo && hi && ring && normals))) return rc;
    if ((rc = search_check_anchor(h, fn, anchor)) || (rc = search_check_counts(h, fn, G, C, K)) || (rc = episode_check_steps(h, fn, max_steps)) ||
        (rc = search_check_box(h, fn, mean0, std0, floor, lo, hi, ring)))
        return rc;
    const size_t E = (size_t)h->E, gc = (size_t)G * C, scores = E * gc;
    if ((rc = search_check_int32(h, fn, std::max(scores, gc * N_AGENTS * 2), "fewer envs, generations or candidates per call")) ||
        (rc = search_check_normals(h, fn, normals, gc * SEARCH_P)) || (rc = episode_check_idle(h, fn)))
        return rc;
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
    search_fill_box(S.B, anchor, mean0, std0, floor, lo, hi, ring);
    S.E = h->E; S.G = G; S.C = C; S.K = K;

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
