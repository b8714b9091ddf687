// The step loop of the receding-horizon rule planner of the Swarm env, shared by the translation units that enqueue it
// (swarm_plan.hip: lookahead and commit of every decision; swarm_search.hip: the lookahead instance as the evaluation of a
// generation of candidate rules; swarm_cemplan.hip: both instances over a table per env).  One copy of the loop, so a search's
// score is the planner's lookahead score with horizon = max_steps, and both are the bits grl_swarm_rules gives from the same state.
// Every including file is compiled with -ffp-contract=off.
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"
#include "swarm_dev.h"
#include "swarm_rule_dev.h"

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
    int stride;                                   // PER_ENV: rows of the table between one env's block and the next (>= n_rules)
};

// One dependent chain per workgroup, as the rules' kernel: latency counts, waves per SIMD do not (cdna_hip_programming.md: occupancy
// hides latency only where there is independent work to switch to; here every wave of the workgroup waits on the same barriers), so
// one wave per SIMD as the second launch bound lets the step loop keep everything in registers.
// Compiled (hipcc -O3, gfx950), lookahead: 118 (exact) / 122 (fast) / 118 (reference divisions) VGPRs, 8 912 bytes of LDS, 4 waves per
// SIMD -- below swarm_rules_kernel's 134 / 138 / 150: it has no reward, action or trace address to keep.  Commit: 140 / 144 / 156 VGPRs,
// 10 192 bytes of LDS (the arg-max's 1 280 bytes of candidate indices), 3 waves per SIMD.  0 bytes of scratch in all six.
// Measured: profiles/swarm_plan_times.json.
// PER_ENV: every env has a table of its own, unit (env, r) reads row env * stride + r of rules and offsets (swarm_cemplan.hip); one
// more multiply-add before the loop, nothing inside it.  Lookahead 118 / 122 / 118 VGPRs, commit 140 / 144 / 156 as without it,
// 0 bytes of scratch.  The two-parameter instances compile to the assembly they had (profiles/swarm_cemplan_isa_same.txt).
template <int MATH, bool COMMIT, bool PER_ENV = false>
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
        const size_t arule = (PER_ENV ? (size_t)aenv * P.stride : 0) + rule_of[ea];
        const double *r = P.rules + arule * 3;
        cancel = r[0]; gain = r[1]; anchor = r[2] != 0.0 ? 1 : 0;          // the host admits 0 and 1 only
        double2 o = reinterpret_cast<const double2 *>(P.offsets)[arule * N_AGENTS + a];
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
