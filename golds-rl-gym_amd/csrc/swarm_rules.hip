// Closed-loop feedback rules on the Swarm env, whole episodes in ONE launch (C ABI: include/goldsrl_swarmrules.h): every (env, rule)
// pair plays its episode from the env's current state, the action of each step computed in the kernel from the positions the step
// before left in LDS.  The reference has no counterpart; the clip is SwarmRunner.transform_actions_for_env
// (agents/paac/emulator_runner.py:113-118) in float64.
//
// Mapping: the replay's (swarm_replay.hip) -- one lane per locust, 4 pairs per 320-lane workgroup, the pairs' agents on the first 40
// lanes; pair p = env * n_rules + rule, a workgroup takes 4 consecutive pairs.  The step is block_step<MATH> of swarm_dev.h and
// nothing else, so a pair's rewards and positions are the bits the replay and the per-step path give for the same action rows.
//
// The start state (x, xa, the pnoise / anoise row in use, elapsed) is read once, and so are the rule's three scalars and the agent
// lane's own offset pair: they stay in registers for the whole episode, the 90 points of each pair in LDS.  Before a step the 40
// agent lanes read their pair's 80 locusts from LDS (every lane of a pair reads the same address: a broadcast) and form the action;
// the HBM traffic of a step is one 8-byte reward per pair and, when asked for, the 160-byte action row per pair and 1 440 bytes of
// positions per pair of the traced env.
//
// The rule's arithmetic (rule_action, swarm_rule_dev.h) is float64, one IEEE operation per statement (the file is compiled with -ffp-contract=off), `/` and sqrt
// correctly rounded in every one of the handle's three math modes: MATH selects block_step only.  The centroid is a SEQUENTIAL sum in
// index order -- the order is part of the contract (goldsrl/_ffi_swarmrules.py:swarm_rule_actions is the same statements in numpy).
//
// The handle's state is read only: nothing here writes x, xa, the noise rows, elapsed, episode or the step's outputs.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_dev.h"
#include "swarm_rule_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_swarmrules.h"

namespace grl {

struct RulesParams {
    const double *x, *xa, *pnoise, *anoise;
    const int32_t *elapsed;
    const double *rules;          // (n_rules, 3): cancel, gain, anchor
    const double *offsets;        // (n_rules, 10, 2)
    double *rewards;              // (E, n_rules, max_steps)
    int32_t *length;              // (E, n_rules)
    uint8_t *finished;            // (E, n_rules)
    double *actions;              // (E, n_rules, max_steps, 10, 2) or null
    double *trace_x, *trace_xa;   // (n_rules, max_steps, 80, 2) (n_rules, max_steps, 10, 2)
    int E, n_rules, max_steps, limit, trace_env;
};

// One dependent chain per workgroup, as the replay: latency counts, waves per SIMD do not, so one wave per SIMD as the second launch
// bound lets the pair loop keep everything in registers.
// Compiled (hipcc -O3, gfx950): 134 (exact) / 138 (fast) / 150 (reference divisions) VGPRs, 0 bytes of scratch, 8 880 bytes of LDS,
// 3 waves per SIMD -- four registers above the replay's 130 / 134 / 146.
// Measured: profiles/swarm_rules_times.json.
template <int MATH>
__global__ __launch_bounds__(SWARM_TPB, 1) void swarm_rules_kernel(RulesParams P) {
    __shared__ SwarmLds L;
    __shared__ int n_end[SWARM_EPB], t_limit[SWARM_EPB];      // steps until max_steps or the TimeLimit ends the pair (0: no pair); the TimeLimit's share
    const int tid = threadIdx.x;
    const int el = tid / N_LOCUSTS, j = tid - el * N_LOCUSTS;
    const int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;   // agent-lane view (valid when tid < 40)
    const bool agent_lane = tid < SWARM_EPB * N_AGENTS;
    const int n_pairs = P.E * P.n_rules;                       // fits: the host checks E * n_rules * max_steps against int32
    const int p0 = blockIdx.x * SWARM_EPB;

    if (tid < SWARM_EPB) {
        const int p = p0 + tid;
        int n = 0, tl = INT_MAX;
        if (p < n_pairs) {
            const int env = p / P.n_rules;
            n = P.max_steps;
            if (P.limit > 0) {                                 // gym TimeLimit: done once elapsed0 + t + 1 >= max_episode_steps
                tl = P.limit - P.elapsed[env];
                if (tl < 1) tl = 1;
            }
            if (tl < n) n = tl;
        }
        n_end[tid] = n;
        t_limit[tid] = tl;
    }

    const int p = p0 + el, pa = p0 + ea;
    const bool active = p < n_pairs, aactive = agent_lane && pa < n_pairs;
    const int env = active ? p / P.n_rules : 0, rule = active ? p - env * P.n_rules : 0;
    const int aenv = aactive ? pa / P.n_rules : 0, arule = aactive ? pa - aenv * P.n_rules : 0;
    const bool traced = active && env == P.trace_env, atraced = aactive && aenv == P.trace_env;

    double xj = 0.5, yj = 0.5, pnx = 0, pny = 0, anx = 0, any = 0;
    double cancel = 0, gain = 0, offx = 0, offy = 0;           // the agent lane's rule, in registers for the whole episode
    int anchor = 0;
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
            const double *r = P.rules + (size_t)arule * 3;
            cancel = r[0]; gain = r[1]; anchor = r[2] != 0.0 ? 1 : 0;      // the host admits 0 and 1 only
            double2 o = reinterpret_cast<const double2 *>(P.offsets)[(size_t)arule * N_AGENTS + a];
            offx = o.x; offy = o.y;
        }
        L.p[ea][N_LOCUSTS + a] = q;
    }
    __syncthreads();

    // bit k: pair k of the workgroup is still playing.  Every lane keeps the same mask: it is updated from L.rew and n_end, which
    // all lanes read after block_step's closing barrier.
    unsigned alive = 0;
#pragma unroll
    for (int k = 0; k < SWARM_EPB; ++k) alive |= n_end[k] > 0 ? 1u << k : 0u;

    for (int t = 0; alive; ++t) {                              // block-uniform
        const bool mine = (alive >> el) & 1u;
        const bool amine = agent_lane && ((alive >> ea) & 1u);
        double actx = 0, acty = 0;
        if (amine) {
            // L.p holds every point of the pair as the closing barrier of the step before (or the one above) left it; the other
            // lanes may already be in block_step, where a locust lane stores the value its slot holds and an agent lane its own slot
            rule_action(L.p[ea], a, cancel, gain, anchor, offx, offy, actx, acty);
            if (P.actions) reinterpret_cast<double2 *>(P.actions)[((size_t)pa * P.max_steps + t) * N_AGENTS + a] = make_double2(actx, acty);
        }
        block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny, false, true);
        if (mine && traced) reinterpret_cast<double2 *>(P.trace_x)[((size_t)rule * P.max_steps + t) * N_LOCUSTS + j] = make_double2(xj, yj);
        if (amine && atraced) reinterpret_cast<double2 *>(P.trace_xa)[((size_t)arule * P.max_steps + t) * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
        unsigned still = alive;
#pragma unroll
        for (int k = 0; k < SWARM_EPB; ++k) {
            if (!((alive >> k) & 1u)) continue;
            const double r = L.rew[k];
            const bool fin = (r >= 0) || (t + 1 >= t_limit[k]);        // multiagent.py:44 + TimeLimit, as the step decides `done`
            if (fin || t + 1 >= n_end[k]) still &= ~(1u << k);
            if (k == el && j == 0) {
                P.rewards[(size_t)p * P.max_steps + t] = r;
                if (!((still >> k) & 1u)) {
                    P.length[p] = t + 1;
                    P.finished[p] = fin ? 1 : 0;
                }
            }
        }
        alive = still;
    }
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_swarm_rules(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t max_steps,
                    int32_t keep_actions, int32_t trace_env) {
    const char *fn = "grl_swarm_rules";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", rules_host && offsets_host)) || (rc = episode_check_count(h, fn, "n_rules", n_rules, 4096)) ||
        (rc = episode_check_steps(h, fn, max_steps)))
        return rc;
    if ((rc = swarm_check_rule_table(h, fn, rules_host, offsets_host, n_rules)) || (rc = episode_check_trace_env(h, fn, trace_env)) ||
        (rc = episode_check_idle(h, fn)))
        return rc;
    const size_t pairs = (size_t)h->E * n_rules, steps = pairs * max_steps, act = keep_actions ? steps : 0;
    const size_t trace = trace_env >= 0 ? (size_t)n_rules * max_steps : 0;
    const size_t largest = std::max(std::max(steps, act * N_AGENTS * 2), trace * N_LOCUSTS * 2);
    if (largest > (size_t)INT32_MAX)
        return fail(h, GRL_E_INVALID, "grl_swarm_rules: an output of " + std::to_string(largest) +
                                          " elements does not fit in int32 (fewer envs, rules or steps per call)");
    hipSetDevice(h->cfg.device_id);
    SwarmRulesState &w = h->srl;
    w.n_rules = 0;
    if ((rc = episode_reserve(h, w.cap_rules, n_rules, {buf(w.rules, 3), buf(w.offsets, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_steps, steps, {buf(w.rewards)})) || (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.length), buf(w.finished)})) ||
        (rc = episode_reserve(h, w.cap_act, act, {buf(w.actions, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_x, N_LOCUSTS * 2), buf(w.trace_xa, N_AGENTS * 2)})))
        return rc;
    if ((rc = swarm_upload_rule_table(h, w.rules, w.offsets, rules_host, offsets_host, n_rules))) return rc;
    GRL_HIP(h, hipMemsetAsync(w.rewards, 0, steps * 8, h->stream));      // rows are defined up to the pair's length; the rest reads as zero
    if ((rc = swarm_zero_kept(h, w.actions, act, w.trace_x, w.trace_xa, trace))) return rc;
    RulesParams P{};
    swarm_start_state(h, P);
    P.rules = w.rules; P.offsets = w.offsets;
    P.rewards = w.rewards; P.length = w.length; P.finished = w.finished; P.actions = act ? w.actions : nullptr;
    P.trace_x = w.trace_x; P.trace_xa = w.trace_xa;
    P.E = h->E; P.n_rules = n_rules; P.max_steps = max_steps; P.limit = h->cfg.max_episode_steps; P.trace_env = trace_env;
    const dim3 grid((unsigned)((pairs + SWARM_EPB - 1) / SWARM_EPB)), block(SWARM_TPB);
    rc = episode_launch(h, [&] {      // the math mode selects block_step, never the rule's own statements
        swarm_math_dispatch(h, [&](auto M) { hipLaunchKernelGGL(swarm_rules_kernel<decltype(M)::value>, grid, block, 0, h->stream, P); });
    });
    if (rc) return rc;
    w.n_rules = n_rules; w.max_steps = max_steps; w.trace_env = trace_env; w.keep_actions = keep_actions ? 1 : 0;
    return GRL_OK;
}

int grl_swarm_rules_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SwarmRulesState &w = h->srl;
    const size_t pairs = (size_t)w.n_rules * h->E, trace = (size_t)w.n_rules * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last run traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"rewards", w.rewards, pairs * w.max_steps * 8}, {"length", w.length, pairs * 4}, {"finished", w.finished, pairs},
        {"actions", w.actions, pairs * w.max_steps * N_AGENTS * 2 * 8, w.keep_actions ? nullptr : "the last run kept no actions (keep_actions was 0)"},
        {"trace_x", w.trace_x, trace * N_LOCUSTS * 2 * 8, untraced}, {"trace_xa", w.trace_xa, trace * N_AGENTS * 2 * 8, untraced}};
    return episode_read(h, "grl_swarm_rules_read", GRL_ENV_SWARM, "Swarm", w.n_rules != 0, "grl_swarm_rules", outs, nullptr, which, host, bytes);
}

}  // extern "C"
