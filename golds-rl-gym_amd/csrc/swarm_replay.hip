// Scripted Swarm episodes in ONE launch (reference scripts/make_swarm_gif.py:62-82 replays the eval monitor's swarm-eval.json
// step by step; C ABI: include/goldsrl_replay.h): every (env, action sequence) pair plays its script from the env's current state.
//
// Mapping: the step's (swarm.hip) -- one lane per locust, 4 pairs per 320-lane workgroup, the pairs' agents on the first 40
// lanes; pair p = env * n_seq + seq, a workgroup takes 4 consecutive pairs.  The arithmetic is block_step<MATH> of swarm_dev.h
// and nothing else, so a pair's rewards and positions are the bits the per-step path gives for the same rows.
//
// The start state (x, xa, the pnoise / anoise row in use, elapsed) is read once.  After that the own locust and the two noise
// pairs stay in registers (after the reset the noise row never changes: quirk Q1), the 90 points of each pair in LDS, and the
// only HBM traffic of a step is the action row (40 lanes x 16 or 8 bytes, asked for one step ahead), one 8-byte reward per pair
// and, for the traced env, 1 440 bytes of positions per pair.  No observation, no done list, no auto-reset.
//
// The handle's state is read only: nothing here writes x, xa, the noise rows, elapsed, episode or the step's outputs.
#include <limits.h>

#include "common.h"
#include "swarm_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_replay.h"

namespace grl {

struct ReplayParams {
    const double *x, *xa, *pnoise, *anoise;
    const int32_t *elapsed;
    const void *actions;          // float64 or float32 rows: (n_seq, max_steps, 10, 2), with per_env (E, n_seq, max_steps, 10, 2)
    const int32_t *seq_len;       // (n_seq) or null
    double *rewards;              // (E, n_seq, max_steps)
    int32_t *length;              // (E, n_seq)
    uint8_t *finished;            // (E, n_seq)
    double *trace_x, *trace_xa;   // (n_seq, max_steps, 80, 2) (n_seq, max_steps, 10, 2)
    int E, n_seq, max_steps, limit, f64, per_env, trace_env;
};

// The kernel is one dependent chain per workgroup (a step's force sums wait for the step before), so latency counts and waves per
// SIMD do not: one wave per SIMD as the second launch bound lets the pair loop keep everything in registers (no scratch).
// Compiled: 130 (exact) / 134 (fast) / 146 (reference divisions) VGPRs, 0 bytes of scratch, 3 waves per SIMD.  Measured
// (profiles/swarm_replay_times.json): one 128-step episode 4.1 ms against 15.5 ms through the SwarmEnv facade; as a batch of 4 096 /
// 32 768 envs x 128 steps 1.30x / 1.48x SLOWER than 128 step launches without the observation, whose 96-register kernel runs
// 5 waves per SIMD -- the replay is for single episodes and small sets of scripts.
template <int MATH>
__global__ __launch_bounds__(SWARM_TPB, 1) void swarm_replay_kernel(ReplayParams P) {
    __shared__ SwarmLds L;
    __shared__ int n_end[SWARM_EPB], t_limit[SWARM_EPB];      // steps until the script or the TimeLimit ends the pair (0: no pair); the TimeLimit's share
    const int tid = threadIdx.x;
    const int el = tid / N_LOCUSTS, j = tid - el * N_LOCUSTS;
    const int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;   // agent-lane view (valid when tid < 40)
    const bool agent_lane = tid < SWARM_EPB * N_AGENTS;
    const int n_pairs = P.E * P.n_seq;                         // fits: the host checks E * n_seq * max_steps against int32
    const int p0 = blockIdx.x * SWARM_EPB;

    if (tid < SWARM_EPB) {
        const int p = p0 + tid;
        int n = 0, tl = INT_MAX;
        if (p < n_pairs) {
            const int env = p / P.n_seq, seq = p - env * P.n_seq;
            n = P.seq_len ? P.seq_len[seq] : P.max_steps;
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
    const int env = active ? p / P.n_seq : 0, seq = active ? p - env * P.n_seq : 0;
    const int aenv = aactive ? pa / P.n_seq : 0, aseq = aactive ? pa - aenv * P.n_seq : 0;
    const bool traced = active && env == P.trace_env, atraced = aactive && aenv == P.trace_env;

    double xj = 0.5, yj = 0.5, pnx = 0, pny = 0, anx = 0, any = 0;
    if (active) {
        double2 q = reinterpret_cast<const double2 *>(P.x)[(size_t)env * N_LOCUSTS + j];
        xj = q.x; yj = q.y;
        double2 n = reinterpret_cast<const double2 *>(P.pnoise)[(size_t)env * N_LOCUSTS + j];
        pnx = n.x; pny = n.y;
    }
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

    // bit k: pair k of the workgroup is still playing.  Every lane keeps the same mask: it is updated from L.rew and n_end, which
    // all lanes read after block_step's closing barrier.
    unsigned alive = 0;
#pragma unroll
    for (int k = 0; k < SWARM_EPB; ++k) alive |= n_end[k] > 0 ? 1u << k : 0u;
    const int a_end = agent_lane ? n_end[ea] : 0;
    // action rows of the agent lane's pair, in (x, y) pairs
    const size_t arow = ((size_t)(P.per_env ? pa : aseq) * P.max_steps) * N_AGENTS + a;
    auto load_action = [&](int t, double &ax, double &ay) {
        if (P.f64) {
            double2 v = reinterpret_cast<const double2 *>(P.actions)[arow + (size_t)t * N_AGENTS];
            ax = v.x; ay = v.y;
        } else {
            float2 v = reinterpret_cast<const float2 *>(P.actions)[arow + (size_t)t * N_AGENTS];
            ax = (double)v.x; ay = (double)v.y;
        }
    };
    double nax = 0, nay = 0;
    if (aactive && a_end > 0) load_action(0, nax, nay);

    for (int t = 0; alive; ++t) {                              // block-uniform
        const bool mine = (alive >> el) & 1u;
        const bool amine = agent_lane && ((alive >> ea) & 1u);
        const double actx = nax, acty = nay;
        if (amine && t + 1 < a_end) load_action(t + 1, nax, nay);      // next step's row, asked for before this step's force sums
        block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny, P.f64 == 0, true);
        if (mine && traced) reinterpret_cast<double2 *>(P.trace_x)[((size_t)seq * P.max_steps + t) * N_LOCUSTS + j] = make_double2(xj, yj);
        if (amine && atraced) reinterpret_cast<double2 *>(P.trace_xa)[((size_t)aseq * P.max_steps + t) * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
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

int grl_swarm_replay(grl_handle *h, const void *actions_host, int32_t actions_f64, int32_t n_seq, int32_t max_steps,
                     const int32_t *seq_len_host, int32_t per_env, int32_t trace_env) {
    const char *fn = "grl_swarm_replay";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SWARM, "Swarm", actions_host)) || (rc = episode_check_count(h, fn, "n_seq", n_seq, 4096)) ||
        (rc = episode_check_steps(h, fn, max_steps)))
        return rc;
    if (seq_len_host) {
        for (int i = 0; i < n_seq; ++i)
            if (seq_len_host[i] < 1 || seq_len_host[i] > max_steps)
                return fail(h, GRL_E_INVALID, "grl_swarm_replay: seq_len[" + std::to_string(i) + "] = " + std::to_string(seq_len_host[i]) +
                                                  " is outside 1.." + std::to_string(max_steps));
    }
    if ((rc = episode_check_trace_env(h, fn, trace_env)) || (rc = episode_check_idle(h, fn))) return rc;
    const size_t pairs = (size_t)h->E * n_seq, steps = pairs * max_steps, trace = trace_env >= 0 ? (size_t)n_seq * max_steps : 0;
    if (steps > (size_t)INT32_MAX || trace * N_LOCUSTS * 2 > (size_t)INT32_MAX)
        return fail(h, GRL_E_INVALID, "grl_swarm_replay: an output of " + std::to_string(std::max(steps, trace * N_LOCUSTS * 2)) +
                                          " elements does not fit in int32 (fewer envs, sequences or steps per call)");
    hipSetDevice(h->cfg.device_id);
    SwarmReplayState &w = h->rpl;
    w.n_seq = 0;
    const size_t act_bytes = (per_env ? pairs : (size_t)n_seq) * max_steps * N_AGENTS * 2 * (actions_f64 ? 8 : 4);
    if ((rc = episode_reserve(h, w.cap_act, act_bytes, {buf(w.actions)})) || (rc = episode_reserve(h, w.cap_seq, n_seq, {buf(w.seq_len)})) ||
        (rc = episode_reserve(h, w.cap_steps, steps, {buf(w.rewards)})) || (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.length), buf(w.finished)})) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_x, N_LOCUSTS * 2), buf(w.trace_xa, N_AGENTS * 2)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.actions, actions_host, act_bytes, hipMemcpyHostToDevice, h->stream));
    if (seq_len_host) GRL_HIP(h, hipMemcpyAsync(w.seq_len, seq_len_host, (size_t)n_seq * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.rewards, 0, steps * 8, h->stream));      // rows are defined up to the pair's length; the rest reads as zero
    if ((rc = swarm_zero_kept(h, nullptr, 0, w.trace_x, w.trace_xa, trace))) return rc;      // a replay keeps no actions: they are its input
    ReplayParams P{};
    swarm_start_state(h, P);
    P.actions = w.actions; P.seq_len = seq_len_host ? w.seq_len : nullptr;
    P.rewards = w.rewards; P.length = w.length; P.finished = w.finished; P.trace_x = w.trace_x; P.trace_xa = w.trace_xa;
    P.E = h->E; P.n_seq = n_seq; P.max_steps = max_steps; P.limit = h->cfg.max_episode_steps;
    P.f64 = actions_f64 ? 1 : 0; P.per_env = per_env ? 1 : 0; P.trace_env = trace_env;
    const dim3 grid((unsigned)((pairs + SWARM_EPB - 1) / SWARM_EPB)), block(SWARM_TPB);
    rc = episode_launch(h, [&] {
        swarm_math_dispatch(h, [&](auto M) { hipLaunchKernelGGL(swarm_replay_kernel<decltype(M)::value>, grid, block, 0, h->stream, P); });
    });
    if (rc) return rc;
    w.n_seq = n_seq; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_swarm_replay_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SwarmReplayState &w = h->rpl;
    const size_t pairs = (size_t)w.n_seq * h->E, trace = (size_t)w.n_seq * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last replay traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"rewards", w.rewards, pairs * w.max_steps * 8}, {"length", w.length, pairs * 4}, {"finished", w.finished, pairs},
        {"trace_x", w.trace_x, trace * N_LOCUSTS * 2 * 8, untraced}, {"trace_xa", w.trace_xa, trace * N_AGENTS * 2 * 8, untraced}};
    return episode_read(h, "grl_swarm_replay_read", GRL_ENV_SWARM, "Swarm", w.n_seq != 0, "grl_swarm_replay", outs, nullptr, which, host, bytes);
}

}  // extern "C"
