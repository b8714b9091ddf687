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
// state and a commit's the bits grl_swarm_step_f64 gives for the same action rows.  The template is in swarm_plan_dev.h: the rule
// search (swarm_search.hip) evaluates its candidates with the lookahead instance.
//
// The handle's state is read only: the plan keeps its own copy of (x, xa) per env and its own clock (SwarmPlanState, common.h); the
// noise rows and elapsed are read from the handle, nothing of it is written.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_plan_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmplan.h"

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
    if ((rc = swarm_upload_rule_table(h, w.rules, w.offsets, rules_host, offsets_host, n_rules)) ||
        (rc = swarm_start_copy(h, w.x, w.xa, w.length, w.finished)))
        return rc;
    GRL_HIP(h, hipMemsetAsync(w.rewards, 0, steps * 8, h->stream));      // rows are defined up to the env's length; the rest reads as zero
    GRL_HIP(h, hipMemsetAsync(w.scores, 0, scores * 8, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.choices, 0xFF, dec * 4, h->stream));     // -1 past the env's last decision
    if ((rc = swarm_zero_kept(h, w.actions, act, w.trace_x, w.trace_xa, trace))) return rc;
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
