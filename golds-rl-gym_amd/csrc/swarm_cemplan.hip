// Search planner on the Swarm env: at every decision each env tunes the rule's five real numbers by a short cross-entropy search over
// lookaheads from where it stands, compares the result with a library of rules, commits the better for `replan` steps and plans again;
// a whole planned episode of every env enqueued in ONE call (C ABI and the scheme, statement by statement:
// include/goldsrl_swarmcemplan.h).  It is the rule planner (swarm_plan.hip) with the rule search (swarm_search.hip) in the place of
// its table, and it is built from their parts:
//   lookahead  swarm_plan_kernel<MATH, false, true> (swarm_plan_dev.h): the planner's loop, reading a table per env.  Env e's block of
//              the working table holds the generation's C candidates, then the R library rows (copied in once, at the first
//              decision).  Generation 0's launch plays all C + R rows -- the library rides along as extra units, so a decision is a
//              chain of G * H + K steps, not (G + 1) * H + K, and the shared loop has no branch for it: it is a longer table --;
//              later generations play the first C rows only.
//   update     swarm_cemplan_update_kernel, one workgroup per env, lane c owning candidate c: rank and refit of the generation
//              before, then the next generation's rows into the env's block; after the last generation the choice between the
//              searched rule and the library's best, the chosen row into the commit's table, the env's new mean.  The candidate,
//              rank and refit statements are the device functions of swarm_search_dev.h and, what knows nothing of Swarm, of
//              search_dev.h, which swarm_search_update_kernel calls too.
//   commit     swarm_plan_kernel<MATH, true, true> over a table of one row per env: the chosen rows of this decision.
// 2 G + 2 launches per decision, D = ceil(max_steps / replan) decisions, all on the handle's stream; nothing is read back between
// them.  The handle's state is read only: the call keeps its own copy of (x, xa) per env and its own clock.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_plan_dev.h"
#include "swarm_search_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmcemplan.h"

namespace grl {

struct CemParams {
    const double *z;                              // (D, G, C, 5): the host's normals, shared by all envs
    const double *lib_rules, *lib_offsets;        // (R, 3) (R, 10, 2)
    const int32_t *length;                        // (E): the call's clock
    const uint8_t *finished;                      // (E)
    double *cur_mean;                             // (E, 5): the env's mean, carried from decision to decision
    double *table_rules, *table_offsets;          // (E, C + R, 3) (E, C + R, 10, 2): the lookahead's table
    const double *look0;                          // (E, D, C + R): generation 0's scores, then the library's
    double *lib_scores;                           // (E, D, R)
    double *cand, *scores;                        // (E, D, G, C, 6) (E, D, G, C)
    int32_t *order;                               // (E, D, G, C)
    double *mean, *std;                           // (E, D, G + 1, 5) each
    int32_t *choices;                             // (E, D)
    double *chosen_rules, *chosen_offsets;        // (E, D, 3) (E, D, 10, 2): the commit's table
    SearchBox B;
    int E, G, C, M, R, D, d, g, max_steps;        // g: the generation whose rows this launch builds (G: none, it chooses)
};

// One workgroup per env, lane c owning candidate c; the workgroup has C lanes rounded up to whole waves (at least 64, so the lanes
// that copy a row's 3 + 20 numbers exist), the lanes past C only keep the barriers.  An ended env's workgroup leaves at once (the
// condition is the env's, so block-uniform): its rows stay the zeros of the call's memsets.  As in the search, the chains are short
// and latency bound -- C LDS reads per lane for the rank, 2 M loads on five lanes for the refit, at most min(R, lanes) LDS reads on
// one lane for the library's best -- so neither occupancy nor bandwidth is the matter; the kernel exists to keep D * G generations on
// the device.  Every index is inside its buffer: rank <= C - 1, order_s[i] < C, the chosen row < C + R, dec < E * D, g <= G.
// Launch bounds 1 024.  Compiled (hipcc -O3, gfx950): 52 VGPRs, 12 376 bytes of LDS (fit 8 192, order 4 096, mean and std 80, the
// chosen row 4 in the 8 of alignment), 0 bytes of scratch.  Measured: profiles/swarm_cemplan_times.json.
__global__ __launch_bounds__(SEARCH_MAX_C) void swarm_cemplan_update_kernel(CemParams P) {
    __shared__ double fit_s[SEARCH_MAX_C];
    __shared__ int order_s[SEARCH_MAX_C];
    __shared__ double mean_s[SEARCH_P], std_s[SEARCH_P];
    __shared__ int row_s;
    const int c = threadIdx.x, lanes = blockDim.x, e = blockIdx.x, C = P.C, G = P.G, R = P.R, g = P.g, T = C + R;
    if (P.finished[e] || P.length[e] >= P.max_steps) return;                   // an ended env takes part in nothing further
    const size_t dec = (size_t)e * P.D + P.d;
    const bool mine = c < C;
    double *trules = P.table_rules + (size_t)e * T * 3, *toffsets = P.table_offsets + (size_t)e * T * N_AGENTS * 2;
    const size_t prev = (dec * G + (g > 0 ? g - 1 : 0)) * C;                   // the rows of the generation before

    if (g == 0) {
        if (c < SEARCH_P) {                       // 1 start: the spread is reset, the mean carried over
            const double m = P.d == 0 ? search_start(P.B, c) : P.cur_mean[(size_t)e * SEARCH_P + c];
            mean_s[c] = m;
            std_s[c] = P.B.std0[c];
            P.mean[dec * (G + 1) * SEARCH_P + c] = m;
            P.std[dec * (G + 1) * SEARCH_P + c] = P.B.std0[c];
            if (P.d == 0) P.cur_mean[(size_t)e * SEARCH_P + c] = m;
        }
        if (P.d == 0)                             // the library, once, behind the candidates of the env's block
            for (int r = c; r < R; r += lanes) {
                for (int k = 0; k < 3; ++k) trules[(size_t)(C + r) * 3 + k] = P.lib_rules[(size_t)r * 3 + k];
                for (int k = 0; k < N_AGENTS * 2; ++k) toffsets[(size_t)(C + r) * N_AGENTS * 2 + k] = P.lib_offsets[(size_t)r * N_AGENTS * 2 + k];
            }
    } else {
        double f = 0.0;
        if (mine) {                               // the fit is the env's own score
            if (g == 1) {
                f = P.look0[dec * T + c];
                P.scores[prev + c] = f;
            } else {
                f = P.scores[prev + c];
            }
        }
        if (g == 1)
            for (int r = c; r < R; r += lanes) P.lib_scores[dec * R + r] = P.look0[dec * T + C + r];
        search_rank(fit_s, order_s, c, C, f, P.order + prev);                  // 7 rank
        if (c < SEARCH_P) {                       // 8 refit
            double m, sd;
            search_refit(P.cand + prev * 6, order_s, P.M, c, P.B.floor[c], m, sd);
            mean_s[c] = m;
            std_s[c] = sd;
            P.mean[(dec * (G + 1) + g) * SEARCH_P + c] = m;
            P.std[(dec * (G + 1) + g) * SEARCH_P + c] = sd;
        }
    }
    __syncthreads();

    if (g < G) {                                  // 2-4: generation g's rows, into the env's block of the table
        if (mine) {
            const size_t row = (dec * G + g) * C + c;
            search_build(P.B, mean_s, std_s, P.z + (((size_t)P.d * G + g) * C + c) * SEARCH_P, c == 0,
                         g == 0 ? nullptr : P.cand + (prev + order_s[0]) * 6, P.cand + row * 6, trules + (size_t)c * 3,
                         toffsets + (size_t)c * N_AGENTS * 2);
        }
        return;
    }

    // 5 choose.  The searched candidate is rank 0 of the last generation; the library's best is the first index of its largest score:
    // lane c scans scores c, c + lanes, ... with a strict >, lane 0 folds the lanes' candidates, a tie going to the smaller index --
    // the same choice as one strict > scan from index 0 (swarm_plan_kernel's arg-max, over this workgroup's lanes).
    const int best_c = order_s[0];
    const double s_best = fit_s[best_c];
    __syncthreads();                              // every lane has read them: fit_s and order_s are free
    const double *ls = P.look0 + dec * T + C;
    double best = 0.0;
    int bi = -1;
    if (c < R) {
        best = ls[c];
        bi = c;
        for (int r = c + lanes; r < R; r += lanes) {
            const double s = ls[r];
            if (s > best) {
                best = s;
                bi = r;
            }
        }
    }
    fit_s[c] = best;
    order_s[c] = bi;
    __syncthreads();
    if (c == 0) {
        const int n = R < lanes ? R : lanes;
        for (int k = 1; k < n; ++k) {
            const double s = fit_s[k];
            const int ci = order_s[k];
            if (s > best || (s == best && ci < bi)) {
                best = s;
                bi = ci;
            }
        }
        const bool searched = bi < 0 || s_best > best;                         // a tie goes to the library
        P.choices[dec] = searched ? R : bi;
        row_s = searched ? best_c : C + bi;
    }
    __syncthreads();
    const int row = row_s;                        // < C: the searched rule, whose rows generation G - 1 left in the table
    if (c < 3) P.chosen_rules[dec * 3 + c] = trules[(size_t)row * 3 + c];
    if (c < N_AGENTS * 2) P.chosen_offsets[dec * N_AGENTS * 2 + c] = toffsets[(size_t)row * N_AGENTS * 2 + c];
    if (row < C && c < SEARCH_P)                  // 6: the env's mean becomes the searched rule's five numbers, bit for bit
        P.cur_mean[(size_t)e * SEARCH_P + c] = P.cand[(prev + best_c) * 6 + search_col(c)];
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_swarm_cemplan(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t anchor,
                      const double *mean0, const double *std0, const double *floor, const double *lo, const double *hi, const double *ring,
                      const double *normals, int32_t horizon, int32_t replan, int32_t G, int32_t C, int32_t M, int32_t max_steps,
                      int32_t keep_actions, int32_t trace_env) {
    const char *fn = "grl_swarm_cemplan";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", mean0 && std0 && floor && lo && hi && ring && normals && (n_rules == 0 || (rules_host && offsets_host)))))
        return rc;
    if (n_rules < 0 || n_rules > 4096) return fail(h, GRL_E_INVALID, "grl_swarm_cemplan: n_rules must be in 0..4096");
    if ((rc = search_check_anchor(h, fn, anchor)) || (rc = search_check_counts(h, fn, G, C, M)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    if (horizon < 1) return fail(h, GRL_E_INVALID, "grl_swarm_cemplan: horizon must be at least 1");
    if (replan < 1 || replan > horizon) return fail(h, GRL_E_INVALID, "grl_swarm_cemplan: replan must be in 1..horizon");
    if ((rc = swarm_check_rule_table(h, fn, rules_host, offsets_host, n_rules)) || (rc = search_check_box(h, fn, mean0, std0, floor, lo, hi, ring)) ||
        (rc = episode_check_trace_env(h, fn, trace_env)))
        return rc;
    const size_t E = (size_t)h->E, D = ((size_t)max_steps + replan - 1) / replan, R = (size_t)n_rules, T = (size_t)C + R;
    const size_t steps = E * max_steps, act = keep_actions ? steps : 0, trace = trace_env >= 0 ? (size_t)max_steps : 0;
    const size_t dec = E * D, gc = dec * G * C, gen = dec * ((size_t)G + 1), look0 = dec * T, lib = dec * R, zn = D * G * C, table = E * T;
    const size_t largest = std::max(std::max(std::max(gc * 6, look0), std::max(dec, table) * N_AGENTS * 2),
                                    std::max(std::max(steps, act * N_AGENTS * 2), std::max(trace * N_LOCUSTS * 2, std::max(zn, gen) * SEARCH_P)));
    if ((rc = search_check_int32(h, fn, largest, "fewer envs, steps, generations, candidates or rules per call")) ||
        (rc = search_check_normals(h, fn, normals, zn * SEARCH_P)) || (rc = episode_check_idle(h, fn)))
        return rc;
    hipSetDevice(h->cfg.device_id);
    SwarmCemPlanState &w = h->scp;
    w.C = 0;
    if ((rc = episode_reserve(h, w.cap_rules, R, {buf(w.lib_rules, 3), buf(w.lib_offsets, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_z, zn, {buf(w.normals, SEARCH_P)})) ||
        (rc = episode_reserve(h, w.cap_envs, E, {buf(w.x, N_LOCUSTS * 2), buf(w.xa, N_AGENTS * 2), buf(w.length), buf(w.pick), buf(w.finished),
                                                 buf(w.cur_mean, SEARCH_P), buf(w.one)})) ||
        (rc = episode_reserve(h, w.cap_steps, steps, {buf(w.rewards)})) || (rc = episode_reserve(h, w.cap_act, act, {buf(w.actions, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_x, N_LOCUSTS * 2), buf(w.trace_xa, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_table, table, {buf(w.table_rules, 3), buf(w.table_offsets, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_dec, dec, {buf(w.choices), buf(w.chosen_rules, 3), buf(w.chosen_offsets, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_look0, look0, {buf(w.look0)})) || (rc = episode_reserve(h, w.cap_lib, lib, {buf(w.lib_scores)})) ||
        (rc = episode_reserve(h, w.cap_gc, gc, {buf(w.cand, 6), buf(w.scores), buf(w.order)})) ||
        (rc = episode_reserve(h, w.cap_gen, gen, {buf(w.mean, SEARCH_P), buf(w.std, SEARCH_P)})))
        return rc;
    if (R) {
        if ((rc = swarm_upload_rule_table(h, w.lib_rules, w.lib_offsets, rules_host, offsets_host, R))) return rc;
        GRL_HIP(h, hipMemsetAsync(w.lib_scores, 0, lib * 8, h->stream));
    }
    GRL_HIP(h, hipMemcpyAsync(w.normals, normals, zn * SEARCH_P * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = swarm_start_copy(h, w.x, w.xa, w.length, w.finished))) return rc;
    GRL_HIP(h, hipMemsetAsync(w.pick, 0, E * 4, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.cur_mean, 0, E * SEARCH_P * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.one, 0, E * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.table_rules, 0, table * 3 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.table_offsets, 0, table * N_AGENTS * 2 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.rewards, 0, steps * 8, h->stream));      // every output is defined up to the env's end; the rest reads as zero
    GRL_HIP(h, hipMemsetAsync(w.choices, 0xFF, dec * 4, h->stream));     // -1 past the env's last decision
    GRL_HIP(h, hipMemsetAsync(w.chosen_rules, 0, dec * 3 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.chosen_offsets, 0, dec * N_AGENTS * 2 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.look0, 0, look0 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.cand, 0, gc * 6 * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.scores, 0, gc * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.order, 0, gc * 4, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.mean, 0, gen * SEARCH_P * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.std, 0, gen * SEARCH_P * 8, h->stream));
    if ((rc = swarm_zero_kept(h, w.actions, act, w.trace_x, w.trace_xa, trace))) return rc;

    CemParams S{};
    S.z = w.normals; S.lib_rules = w.lib_rules; S.lib_offsets = w.lib_offsets; S.length = w.length; S.finished = w.finished;
    S.cur_mean = w.cur_mean; S.table_rules = w.table_rules; S.table_offsets = w.table_offsets; S.look0 = w.look0; S.lib_scores = w.lib_scores;
    S.cand = w.cand; S.scores = w.scores; S.order = w.order; S.mean = w.mean; S.std = w.std;
    S.choices = w.choices; S.chosen_rules = w.chosen_rules; S.chosen_offsets = w.chosen_offsets;
    search_fill_box(S.B, anchor, mean0, std0, floor, lo, hi, ring);
    S.E = h->E; S.G = G; S.C = C; S.M = M; S.R = n_rules; S.D = (int)D; S.max_steps = max_steps;

    PlanParams P{};                               // the lookaheads and the commit share the state, the clock and the outputs of the steps
    swarm_start_state(h, P);
    P.x = w.x; P.xa = w.xa; P.wx = w.x; P.wxa = w.xa;
    P.length = w.length; P.finished = w.finished;
    P.rewards = w.rewards; P.actions = act ? w.actions : nullptr; P.trace_x = w.trace_x; P.trace_xa = w.trace_xa;
    P.E = h->E; P.horizon = horizon; P.replan = replan; P.max_steps = max_steps;
    P.limit = h->cfg.max_episode_steps; P.trace_env = trace_env;
    const dim3 update((unsigned)E), lanes((unsigned)std::max<size_t>(64, ((size_t)C + 63) / 64 * 64));
    const dim3 look_all((unsigned)((E * T + SWARM_EPB - 1) / SWARM_EPB)), look_cand((unsigned)((E * C + SWARM_EPB - 1) / SWARM_EPB));
    const dim3 commit((unsigned)((E + SWARM_EPB - 1) / SWARM_EPB)), block(SWARM_TPB);
    rc = episode_launch(h, [&] {                  // the math mode selects block_step, never the rule's or the search's statements
        swarm_math_dispatch(h, [&](auto MM) {
            for (int d = 0; d < (int)D; ++d) {
                S.d = d;
                P.rules = w.table_rules; P.offsets = w.table_offsets; P.stride = (int)T; P.choices = nullptr;
                for (int g = 0; g <= G; ++g) {
                    S.g = g;
                    hipLaunchKernelGGL(swarm_cemplan_update_kernel, update, lanes, 0, h->stream, S);
                    if (g == G) break;
                    if (g == 0) {                 // the candidates and the library: (E, D, C + R) scores
                        P.n_rules = (int)T; P.D = (int)D; P.d = d; P.scores = w.look0;
                    } else {                      // the candidates: (E, D * G, C) scores
                        P.n_rules = C; P.D = (int)D * G; P.d = d * G + g; P.scores = w.scores;
                    }
                    hipLaunchKernelGGL((swarm_plan_kernel<decltype(MM)::value, false, true>), g == 0 ? look_all : look_cand, block, 0, h->stream, P);
                }
                // the commit's table: this decision's chosen rows, one per env; its arg-max over one score picks row 0
                P.rules = w.chosen_rules + (size_t)d * 3; P.offsets = w.chosen_offsets + (size_t)d * N_AGENTS * 2; P.stride = (int)D;
                P.n_rules = 1; P.D = 1; P.d = 0; P.scores = w.one; P.choices = w.pick;
                hipLaunchKernelGGL((swarm_plan_kernel<decltype(MM)::value, true, true>), commit, block, 0, h->stream, P);
            }
        });
    });
    if (rc) return rc;
    w.n_rules = n_rules; w.max_steps = max_steps; w.decisions = (int)D; w.G = G; w.C = C; w.trace_env = trace_env; w.keep_actions = keep_actions ? 1 : 0;
    return GRL_OK;
}

int grl_swarm_cemplan_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SwarmCemPlanState &w = h->scp;
    const size_t E = (size_t)h->E, steps = E * w.max_steps, dec = E * w.decisions, trace = (size_t)w.max_steps;
    const size_t gc = dec * w.G * w.C, gen = dec * ((size_t)w.G + 1);
    const char *untraced = w.trace_env < 0 ? "the last run traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"rewards", w.rewards, steps * 8}, {"length", w.length, E * 4}, {"finished", w.finished, E},
        {"choices", w.choices, dec * 4}, {"chosen_rules", w.chosen_rules, dec * 3 * 8}, {"chosen_offsets", w.chosen_offsets, dec * N_AGENTS * 2 * 8},
        {"lib_scores", w.lib_scores, dec * w.n_rules * 8, w.n_rules ? nullptr : "the last run had no library (n_rules was 0)"},
        {"candidates", w.cand, gc * 6 * 8}, {"scores", w.scores, gc * 8}, {"order", w.order, gc * 4},
        {"mean", w.mean, gen * SEARCH_P * 8}, {"std", w.std, gen * SEARCH_P * 8},
        {"actions", w.actions, steps * N_AGENTS * 2 * 8, w.keep_actions ? nullptr : "the last run kept no actions (keep_actions was 0)"},
        {"trace_x", w.trace_x, trace * N_LOCUSTS * 2 * 8, untraced}, {"trace_xa", w.trace_xa, trace * N_AGENTS * 2 * 8, untraced}};
    return episode_read(h, "grl_swarm_cemplan_read", GRL_ENV_SWARM, "Swarm", w.C != 0, "grl_swarm_cemplan", outs, nullptr, which, host, bytes);
}

}  // extern "C"
