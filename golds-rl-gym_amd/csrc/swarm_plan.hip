// Receding-horizon rule planner on the Swarm env, a whole planned episode enqueued in ONE call (C ABI: include/goldsrl_swarmplan.h):
// at every decision each env plays every rule of the table `horizon` steps ahead from where it stands, takes the rule with the best
// sum, commits it for `replan` steps and plans again.  SwarmEnv.t stops at 10 after the burn-in (quirk Q1), so every step reuses one
// noise row and the env is deterministic from a given state: the lookahead plays the true model and knows nothing a policy could not.
// The reference has no counterpart.
//
// Two kernels per decision, D = ceil(max_steps / replan) decisions, all on the handle's stream; nothing is read back between them.
//   lookahead  swarm_rules_kernel's mapping (swarm_rules.hip): one lane per locust, 4 (env, rule) pairs per 320-lane workgroup, the
//              state in registers and LDS, the rule's scalars in registers.  Its only HBM output is one 8-byte score per pair: the
//              float64 sum of the pair's rewards in step order.
//   commit     4 envs per workgroup: the arg-max of the env's n_rules scores (the first index of the largest), then the same step
//              loop under the chosen rule for `replan` steps, then the working state is stored for the next decision.
// They are the two instances of one template (COMMIT): what a unit of the workgroup is (a pair or an env), how many steps it plays
// and what it writes differ, the loop does not.  The step is block_step<MATH> (swarm_dev.h) and the action rule_action
// (swarm_rule_dev.h), both as swarm_rules_kernel uses them, so a lookahead's rewards are the bits grl_swarm_rules gives from the same
// state and a commit's the bits grl_swarm_step_f64 gives for the same action rows.
//
// The handle's state is read only: the plan keeps its own copy of (x, xa) per env and its own clock (SwarmPlanState, common.h); the
// noise rows and elapsed are read from the handle, nothing of it is written.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_dev.h"
#include "swarm_rule_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmplan.h"

namespace grl {

struct PlanParams {
    const double *x, *xa, *pnoise, *anoise;       // x, xa: the plan's working copy; the noise rows: the handle's
    const int32_t *elapsed;                       // the handle's, as the call found it
    const double *rules;                          // (n_rules, 3): cancel, gain, anchor
    const double *offsets;                        // (n_rules, 10, 2)
    double *wx, *wxa;                             // x, xa again, for the commit's store
    int32_t *length;                              // (E): steps committed so far
    uint8_t *finished;                            // (E)
    double *scores;                               // (E, D, n_rules)
    int32_t *choices;                             // (E, D)
    double *rewards;                              // (E, max_steps)
    double *actions;                              // (E, max_steps, 10, 2) or null
    double *trace_x, *trace_xa;                   // (max_steps, 80, 2) (max_steps, 10, 2)
    int E, n_rules, horizon, replan, max_steps, limit, trace_env, D, d;
};

// One dependent chain per workgroup, as the rules' kernel: latency counts, waves per SIMD do not (cdna_hip_programming.md: occupancy
// hides latency only where there is independent work to switch to; here every wave of the workgroup waits on the same barriers), so
// one wave per SIMD as the second launch bound lets the step loop keep everything in registers.
// Compiled (hipcc -O3, gfx950), lookahead: 118 (exact) / 122 (fast) / 118 (reference divisions) VGPRs, 8 912 bytes of LDS, 4 waves per
// SIMD -- below swarm_rules_kernel's 134 / 138 / 150: it has no reward, action or trace address to keep.  Commit: 140 / 144 / 156 VGPRs,
// 10 192 bytes of LDS (the arg-max's 1 280 bytes of candidate indices), 3 waves per SIMD.  0 bytes of scratch in all six.
// Measured: profiles/swarm_plan_times.json.
template <int MATH, bool COMMIT>
__global__ __launch_bounds__(SWARM_TPB, 1) void swarm_plan_kernel(PlanParams P) {
    __shared__ SwarmLds L;
    __shared__ int n_end[SWARM_EPB], t_limit[SWARM_EPB];      // steps until this call's share or the TimeLimit ends the unit (0: none); the TimeLimit's share
    __shared__ int t_first[SWARM_EPB], rule_of[SWARM_EPB];    // the unit's clock at its first step; its rule
    const int tid = threadIdx.x;
    const int el = tid / N_LOCUSTS, j = tid - el * N_LOCUSTS;
    const int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;   // agent-lane view (valid when tid < 40)
    const bool agent_lane = tid < SWARM_EPB * N_AGENTS;
    const int n_units = COMMIT ? P.E : P.E * P.n_rules;       // fits: the host checks E * D * n_rules against int32
    const int u0 = blockIdx.x * SWARM_EPB;
    const int u = u0 + el, ua = u0 + ea;
    const bool active = u < n_units, aactive = agent_lane && ua < n_units;
    const int env = active ? (COMMIT ? u : u / P.n_rules) : 0;
    const int aenv = aactive ? (COMMIT ? ua : ua / P.n_rules) : 0;

    if constexpr (COMMIT) {
        // The first index of the largest score: lane j scans rules j, j + 80, ... with a strict >, lane 0 then folds the 80 candidates,
        // a tie going to the smaller index.  The same choice as one strict > scan from rule 0.
        __shared__ int cand[SWARM_EPB][N_LOCUSTS];
        const double *sc = P.scores + ((size_t)env * P.D + P.d) * P.n_rules;
        double best = 0;
        int bi = -1;
        if (active && j < P.n_rules) {
            best = sc[j];
            bi = j;
            for (int r = j + N_LOCUSTS; r < P.n_rules; r += N_LOCUSTS) {
                const double s = sc[r];
                if (s > best) {
                    best = s;
                    bi = r;
                }
            }
        }
        L.en[el][j] = best;
        cand[el][j] = bi;
        __syncthreads();
        if (j == 0) {
            for (int k = 1; k < N_LOCUSTS; ++k) {
                const int ci = cand[el][k];
                if (ci < 0) break;                             // lanes past n_rules hold nothing, and so do all after them
                const double s = L.en[el][k];
                if (s > best || (s == best && ci < bi)) {
                    best = s;
                    bi = ci;
                }
            }
            rule_of[el] = bi < 0 ? 0 : bi;
        }
    }

    if (tid < SWARM_EPB) {
        const int uu = u0 + tid;
        int n = 0, tl = INT_MAX, t0 = 0;
        if (!COMMIT) rule_of[tid] = 0;
        if (uu < n_units) {
            const int e = COMMIT ? uu : uu / P.n_rules;
            t0 = P.length[e];
            if (!P.finished[e] && t0 < P.max_steps) {         // an ended env takes part in nothing further
                n = COMMIT ? min(P.replan, P.max_steps - t0) : P.horizon;      // the lookahead is not shortened by max_steps
                if (P.limit > 0) {                             // gym TimeLimit: done once elapsed + 1 >= max_episode_steps
                    tl = P.limit - (P.elapsed[e] + t0);
                    if (tl < 1) tl = 1;
                }
                if (tl < n) n = tl;
            }
            if (!COMMIT) rule_of[tid] = uu - e * P.n_rules;
        }
        n_end[tid] = n;
        t_limit[tid] = tl;
        t_first[tid] = t0;
    }

    double xj = 0.5, yj = 0.5, pnx = 0, pny = 0, anx = 0, any = 0;
    if (active) {
        double2 q = reinterpret_cast<const double2 *>(P.x)[(size_t)env * N_LOCUSTS + j];
        xj = q.x; yj = q.y;
        double2 n = reinterpret_cast<const double2 *>(P.pnoise)[(size_t)env * N_LOCUSTS + j];
        pnx = n.x; pny = n.y;
    }
    L.p[el][j] = make_double2(xj, yj);                         // the rule reads the locusts before the first block_step stores them
    if (agent_lane) {
        double2 q = make_double2(0.5, 0.5);
        if (aactive) {
            q = reinterpret_cast<const double2 *>(P.xa)[(size_t)aenv * N_AGENTS + a];
            double2 n = reinterpret_cast<const double2 *>(P.anoise)[(size_t)aenv * N_AGENTS + a];
            anx = n.x; any = n.y;
        }
        L.p[ea][N_LOCUSTS + a] = q;
    }
    __syncthreads();

    double cancel = 0, gain = 0, offx = 0, offy = 0;           // the agent lane's rule, in registers for the whole loop
    int anchor = 0;
    if (aactive) {
        const int arule = rule_of[ea];
        const double *r = P.rules + (size_t)arule * 3;
        cancel = r[0]; gain = r[1]; anchor = r[2] != 0.0 ? 1 : 0;          // the host admits 0 and 1 only
        double2 o = reinterpret_cast<const double2 *>(P.offsets)[(size_t)arule * N_AGENTS + a];
        offx = o.x; offy = o.y;
    }
    const int rule = rule_of[el], t0 = t_first[el], at0 = agent_lane ? t_first[ea] : 0;
    const bool traced = COMMIT && active && env == P.trace_env, atraced = COMMIT && aactive && aenv == P.trace_env;
    const bool played = n_end[el] > 0;

    // bit k: unit k of the workgroup is still playing.  Every lane keeps the same mask: it is updated from L.rew and n_end, which
    // all lanes read after block_step's closing barrier.
    unsigned alive = 0;
#pragma unroll
    for (int k = 0; k < SWARM_EPB; ++k) alive |= n_end[k] > 0 ? 1u << k : 0u;
    if (COMMIT && played && j == 0) P.choices[(size_t)env * P.D + P.d] = rule;

    double score = 0.0;                                        // s = 0.0; s = s + r_t, in step order
    for (int t = 0; alive; ++t) {                              // block-uniform
        const bool mine = (alive >> el) & 1u;
        const bool amine = agent_lane && ((alive >> ea) & 1u);
        double actx = 0, acty = 0;
        if (amine) {
            // L.p holds every point of the unit as the closing barrier of the step before (or the one above) left it; the other
            // lanes may already be in block_step, where a locust lane stores the value its slot holds and an agent lane its own slot
            rule_action(L.p[ea], a, cancel, gain, anchor, offx, offy, actx, acty);
            if (COMMIT && P.actions)
                reinterpret_cast<double2 *>(P.actions)[((size_t)aenv * P.max_steps + at0 + t) * N_AGENTS + a] = make_double2(actx, acty);
        }
        block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny, false, true);
        if (mine && traced) reinterpret_cast<double2 *>(P.trace_x)[((size_t)t0 + t) * N_LOCUSTS + j] = make_double2(xj, yj);
        if (amine && atraced) reinterpret_cast<double2 *>(P.trace_xa)[((size_t)at0 + t) * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
        unsigned still = alive;
#pragma unroll
        for (int k = 0; k < SWARM_EPB; ++k) {
            if (!((alive >> k) & 1u)) continue;
            const double r = L.rew[k];
            const bool fin = (r >= 0) || (t + 1 >= t_limit[k]);        // multiagent.py:44 + TimeLimit, as the step decides `done`
            if (fin || t + 1 >= n_end[k]) still &= ~(1u << k);
            if (k == el && j == 0) {
                const bool over = !((still >> k) & 1u);
                if (COMMIT) {
                    P.rewards[(size_t)env * P.max_steps + t0 + t] = r;
                    if (over) {
                        P.length[env] = t0 + t + 1;
                        P.finished[env] = fin ? 1 : 0;
                    }
                } else {
                    score = score + r;
                    if (over) P.scores[((size_t)env * P.D + P.d) * P.n_rules + rule] = score;
                }
            }
        }
        alive = still;
    }

    if (COMMIT) {
        // The state the next decision starts from.  An env that ended inside this commit has played on with zero actions since: its
        // state is stored too and never read again.
        if (played) reinterpret_cast<double2 *>(P.wx)[(size_t)env * N_LOCUSTS + j] = make_double2(xj, yj);
        if (aactive && n_end[ea] > 0) reinterpret_cast<double2 *>(P.wxa)[(size_t)aenv * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
    }
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_swarm_plan(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t horizon, int32_t replan,
                   int32_t max_steps, int32_t keep_actions, int32_t trace_env) {
    const char *fn = "grl_swarm_plan";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", rules_host && offsets_host)) || (rc = episode_check_count(h, fn, "n_rules", n_rules, 4096)) ||
        (rc = episode_check_steps(h, fn, max_steps)))
        return rc;
    if (horizon < 1) return fail(h, GRL_E_INVALID, "grl_swarm_plan: horizon must be at least 1");      // episode_check_steps' test, its own noun
    if (replan < 1 || replan > horizon) return fail(h, GRL_E_INVALID, "grl_swarm_plan: replan must be in 1..horizon");
    if ((rc = swarm_check_rule_table(h, fn, rules_host, offsets_host, n_rules)) || (rc = episode_check_trace_env(h, fn, trace_env)) ||
        (rc = episode_check_idle(h, fn)))
        return rc;
    const size_t E = (size_t)h->E, D = ((size_t)max_steps + replan - 1) / replan;
    const size_t steps = E * max_steps, act = keep_actions ? steps : 0, trace = trace_env >= 0 ? (size_t)max_steps : 0;
    const size_t dec = E * D, scores = dec * n_rules;
    const size_t largest = std::max(std::max(scores, act * N_AGENTS * 2), std::max(steps, trace * N_LOCUSTS * 2));
    if (largest > (size_t)INT32_MAX)
        return fail(h, GRL_E_INVALID, "grl_swarm_plan: an output of " + std::to_string(largest) +
                                          " elements does not fit in int32 (fewer envs, rules or steps per call)");
    hipSetDevice(h->cfg.device_id);
    SwarmPlanState &w = h->spl;
    w.n_rules = 0;
    if ((rc = episode_reserve(h, w.cap_rules, n_rules, {buf(w.rules, 3), buf(w.offsets, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_envs, E, {buf(w.x, N_LOCUSTS * 2), buf(w.xa, N_AGENTS * 2), buf(w.length), buf(w.finished)})) ||
        (rc = episode_reserve(h, w.cap_steps, steps, {buf(w.rewards)})) || (rc = episode_reserve(h, w.cap_act, act, {buf(w.actions, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_x, N_LOCUSTS * 2), buf(w.trace_xa, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_dec, dec, {buf(w.choices)})) || (rc = episode_reserve(h, w.cap_scores, scores, {buf(w.scores)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.rules, rules_host, (size_t)n_rules * 3 * 8, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.offsets, offsets_host, (size_t)n_rules * N_AGENTS * 2 * 8, hipMemcpyHostToDevice, h->stream));
    // the working copy starts as the handle's positions; the plan's clock at zero
    GRL_HIP(h, hipMemcpyAsync(w.x, h->sw.x, E * N_LOCUSTS * 2 * 8, hipMemcpyDeviceToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.xa, h->sw.xa, E * N_AGENTS * 2 * 8, hipMemcpyDeviceToDevice, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.length, 0, E * 4, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.finished, 0, E, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.rewards, 0, steps * 8, h->stream));      // rows are defined up to the env's length; the rest reads as zero
    GRL_HIP(h, hipMemsetAsync(w.scores, 0, scores * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.choices, 0xFF, dec * 4, h->stream));     // -1 past the env's last decision
    if (act) GRL_HIP(h, hipMemsetAsync(w.actions, 0, act * N_AGENTS * 2 * 8, h->stream));
    if (trace) {
        GRL_HIP(h, hipMemsetAsync(w.trace_x, 0, trace * N_LOCUSTS * 2 * 8, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_xa, 0, trace * N_AGENTS * 2 * 8, h->stream));
    }
    PlanParams P{};
    swarm_start_state(h, P);
    P.x = w.x; P.xa = w.xa; P.wx = w.x; P.wxa = w.xa;
    P.rules = w.rules; P.offsets = w.offsets;
    P.length = w.length; P.finished = w.finished; P.scores = w.scores; P.choices = w.choices;
    P.rewards = w.rewards; P.actions = act ? w.actions : nullptr; P.trace_x = w.trace_x; P.trace_xa = w.trace_xa;
    P.E = h->E; P.n_rules = n_rules; P.horizon = horizon; P.replan = replan; P.max_steps = max_steps;
    P.limit = h->cfg.max_episode_steps; P.trace_env = trace_env; P.D = (int)D;
    const dim3 look((unsigned)((E * n_rules + SWARM_EPB - 1) / SWARM_EPB)), commit((unsigned)((E + SWARM_EPB - 1) / SWARM_EPB)), block(SWARM_TPB);
    rc = episode_launch(h, [&] {      // the math mode selects block_step, never the rule's own statements
        swarm_math_dispatch(h, [&](auto M) {
            for (int d = 0; d < (int)D; ++d) {
                P.d = d;
                hipLaunchKernelGGL((swarm_plan_kernel<decltype(M)::value, false>), look, block, 0, h->stream, P);
                hipLaunchKernelGGL((swarm_plan_kernel<decltype(M)::value, true>), commit, block, 0, h->stream, P);
            }
        });
    });
    if (rc) return rc;
    w.n_rules = n_rules; w.max_steps = max_steps; w.decisions = (int)D; w.trace_env = trace_env; w.keep_actions = keep_actions ? 1 : 0;
    return GRL_OK;
}

int grl_swarm_plan_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SwarmPlanState &w = h->spl;
    const size_t E = (size_t)h->E, steps = E * w.max_steps, dec = E * w.decisions, trace = (size_t)w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last run traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"rewards", w.rewards, steps * 8}, {"length", w.length, E * 4}, {"finished", w.finished, E},
        {"choices", w.choices, dec * 4}, {"scores", w.scores, dec * w.n_rules * 8},
        {"actions", w.actions, steps * N_AGENTS * 2 * 8, w.keep_actions ? nullptr : "the last run kept no actions (keep_actions was 0)"},
        {"trace_x", w.trace_x, trace * N_LOCUSTS * 2 * 8, untraced}, {"trace_xa", w.trace_xa, trace * N_AGENTS * 2 * 8, untraced}};
    return episode_read(h, "grl_swarm_plan_read", GRL_ENV_SWARM, "Swarm", w.n_rules != 0, "grl_swarm_plan", outs, nullptr, which, host, bytes);
}

}  // extern "C"
