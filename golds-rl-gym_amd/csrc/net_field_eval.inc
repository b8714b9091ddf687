// Evaluation of ConvPolicyVFieldNetwork on a Swarm handle, whole episodes in ONE launch (C ABI: include/goldsrl_fieldeval.h); included
// by net_field.hip behind net_field_rollout.inc.  Every env of the handle plays its episode from its current state; the policy acts
// on the compact observation the kernel forms from the positions the step before left in LDS, so an episode never leaves its CU.
//
// Nothing here restates arithmetic: the observation is swarm_mean_x / swarm_point_bin / swarm_point_pos (swarm_dev.h, the statements
// of the step kernel's observation), the forward field_env_forward (the fused rollout step's), the draw and the norm clip
// field_sample_one / field_norm_clip, the step block_step<MATH> -- so the greedy float64-row episode is, bit for bit, the host loop
// predict_swarm -> transform_actions -> float64 step, and the drawn float32-row episode is the training rollout's up to the first done.
//
// Mapping: one workgroup of SWARM_TPB lanes per env.  The env sits in slot 0 of a SwarmLds; slots 1..3 hold the idle pair of the last
// partial workgroup of the replay and rules kernels (every point at (0.5, 0.5), no noise, no action), so block_step runs unchanged.
// All five waves take part in the forward: every activation is one lane's sequential sum, two agents' head columns per wave.  One env
// is one dependent chain (observation -> forward -> action -> step), and eval sets are small: a second env in the workgroup would
// lengthen the chain's forward by sharing its lanes and save nothing but idle waves that have no other work to go to.
//
// The start state (x, xa, the pnoise / anoise row in use, elapsed) is read once; the locust stays in registers, the points, the 200
// observation bytes, the ten actions and the activations in LDS.  Parameters and head columns come from global memory (L2).  A step's
// HBM traffic is one float64 reward, the 160-byte action row when kept, and the trace rows of the traced env.
//
// LDS: sizeof(SwarmLds) + 208 observation bytes + 80 action bytes + the forward's floats (field_fwd_floats), all in the dynamic region
// so that its base stays 16-byte aligned; past 64 KB the geometry is refused before the launch.
//
// The handle and the net are read only: no env state, observation, record, counter, parameter or rollout buffer is written.
#include <limits.h>

namespace grl {

constexpr int FE_OBS_BYTES = 208;      // locust_bins 160, agent_bins 20, positions 20, padded to 16
constexpr int FE_ACT_BYTES = N_AGENTS * 8;
constexpr size_t FE_HEAD_BYTES = sizeof(SwarmLds) + FE_OBS_BYTES + FE_ACT_BYTES;
static_assert(sizeof(SwarmLds) % 16 == 0 && FE_HEAD_BYTES % 16 == 0, "the carve offsets of field_eval_kernel's LDS");

struct FieldEvalArgs : FieldFwdArgs {
    const double *x, *xa, *pnoise, *anoise;      // swarm_start_state
    const int32_t *elapsed;
    uint64_t seed;
    uint32_t env_off, counter;
    int max_steps, limit, trace_env, greedy, act32;
    double *rewards;                              // (E, max_steps)
    int32_t *length;                              // (E)
    uint8_t *finished;                            // (E)
    double *actions;                              // (E, max_steps, 10, 2) or null
    float *tr_mu, *tr_sigma, *tr_value, *tr_raw;  // the traced env: (max_steps,10,2) x2, (max_steps), (max_steps,10,2)
    uint8_t *tr_lb, *tr_ab, *tr_pos;              // (max_steps,80,2) (max_steps,10,2) x2: the observation each step acted on
    double *tr_x, *tr_xa;                         // (max_steps,80,2) (max_steps,10,2): the positions after each step
};

// One dependent chain per workgroup: latency counts, waves per SIMD do not (second launch bound 1, as the rules kernel).
// Compiled (hipcc -O3 --offload-arch=gfx950): 173 (exact) / 175 (fast) / 175 (reference divisions) VGPRs, 0 bytes of scratch each, no static
// LDS; dynamic LDS 9 136 bytes (SwarmLds 8 848, observation 208, actions 80) + the forward's floats: 22 516 at G = 20, F = 5, L = 2.
// The kernel's arguments with every address derived from them exceed the scalar file, so about 240 scalars live in lanes of four
// VGPRs (v_writelane / v_readlane, no memory traffic).  Without the opaque lane index below the per-lane addresses of the forward
// were hoisted out of the episode loop: 256 VGPRs and 340 bytes of scratch.
// Measured (profiles/field_eval_times.json, 128 steps): 10.6 ms at 1 and at 64 envs, 169 ms at 4 096 -- 83 us per step on the chain, of
// which block_step is ~35 (the rules kernel's step); the rest is the forward, whose dense layers are chains of L2 loads (eight in flight).
template <int MATH>
__global__ __launch_bounds__(SWARM_TPB, 1) void field_eval_kernel(FieldEvalArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_lds[];
    SwarmLds &L = *reinterpret_cast<SwarmLds *>(fe_lds);
    uint8_t *lb = fe_lds + sizeof(SwarmLds), *ab = lb + N_LOCUSTS * 2, *ps = ab + N_AGENTS * 2;
    float2 *act = reinterpret_cast<float2 *>(fe_lds + sizeof(SwarmLds) + FE_OBS_BYTES);
    float *fl = reinterpret_cast<float *>(fe_lds + FE_HEAD_BYTES);
    const int tid = threadIdx.x, env = blockIdx.x;
    const int el = tid / N_LOCUSTS, j = tid - el * N_LOCUSTS;
    const int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;   // agent-lane view (valid when tid < 40)
    const bool agent_lane = tid < SWARM_EPB * N_AGENTS;
    const bool mine = el == 0, amine = tid < N_AGENTS;         // the lanes of the env's own locusts and agents
    const bool traced = env == P.trace_env;
    const size_t S = (size_t)P.max_steps;

    int n_end = P.max_steps, t_limit = INT_MAX;                // steps until max_steps or the TimeLimit ends the episode; the TimeLimit's share
    if (P.limit > 0) {                                         // gym TimeLimit: done once elapsed0 + t + 1 >= max_episode_steps
        t_limit = P.limit - P.elapsed[env];
        if (t_limit < 1) t_limit = 1;
    }
    if (t_limit < n_end) n_end = t_limit;

    double xj = 0.5, yj = 0.5, pnx = 0, pny = 0, anx = 0, any = 0;
    if (mine) {
        double2 q = reinterpret_cast<const double2 *>(P.x)[(size_t)env * N_LOCUSTS + j];
        xj = q.x; yj = q.y;
        double2 n = reinterpret_cast<const double2 *>(P.pnoise)[(size_t)env * N_LOCUSTS + j];
        pnx = n.x; pny = n.y;
    }
    L.p[el][j] = make_double2(xj, yj);                         // the observation reads the locusts before the first block_step stores them
    if (agent_lane) {
        double2 q = make_double2(0.5, 0.5);
        if (amine) {
            q = reinterpret_cast<const double2 *>(P.xa)[(size_t)env * N_AGENTS + a];
            double2 n = reinterpret_cast<const double2 *>(P.anoise)[(size_t)env * N_AGENTS + a];
            anx = n.x; any = n.y;
        }
        L.p[ea][N_LOCUSTS + a] = q;
    }
    __syncthreads();

    for (int t = 0;; ++t) {                                    // uniform: see `fin` below
        // ---- the observation of the state as it stands: L.p[0] holds every point behind the barrier above / block_step's closing one
        if (tid == 0) L.meanx[0] = swarm_mean_x(L.p[0]);
        __syncthreads();
        if (mine) {
            int cx, cy;
            const uint16_t bin = swarm_point_bin(xj, yj, L.meanx[0], P.G, cx, cy);
            reinterpret_cast<uint16_t *>(lb)[j] = bin;
            if (traced) reinterpret_cast<uint16_t *>(P.tr_lb)[(size_t)t * N_LOCUSTS + j] = bin;
        }
        if (amine) {
            const double2 q = L.p[0][N_LOCUSTS + a];
            int cx, cy;
            const uint16_t bin = swarm_point_bin(q.x, q.y, L.meanx[0], P.G, cx, cy), pos = swarm_point_pos(cx, cy, P.G);
            reinterpret_cast<uint16_t *>(ab)[a] = bin;
            reinterpret_cast<uint16_t *>(ps)[a] = pos;
            if (traced) {
                reinterpret_cast<uint16_t *>(P.tr_ab)[(size_t)t * N_AGENTS + a] = bin;
                reinterpret_cast<uint16_t *>(P.tr_pos)[(size_t)t * N_AGENTS + a] = pos;
            }
        }
        // ---- image, trunk, towers, heads; the forward's first barrier orders the bytes above
        int ft = tid;
        asm volatile("" : "+v"(ft));      // opaque per step: else every per-lane address of the forward is hoisted out of the episode loop and spilled
        field_env_forward<8>(P, lb, ab, ps, fl, ft, SWARM_TPB, [&](int ag, float2 m, float2 s, float vs) {
            float2 raw = m, clipped;
            if (P.greedy) clipped = field_norm_clip(m);
            else field_sample_one(m, s, P.seed, (uint32_t)env + P.env_off, P.counter + (uint32_t)t, (uint32_t)ag, &raw, &clipped);
            act[ag] = clipped;
            if (traced) {
                const size_t i = (size_t)t * N_AGENTS + ag;
                reinterpret_cast<float2 *>(P.tr_mu)[i] = m;
                reinterpret_cast<float2 *>(P.tr_sigma)[i] = s;
                reinterpret_cast<float2 *>(P.tr_raw)[i] = raw;
                if (ag == 0) P.tr_value[t] = vs;
            }
        });
        __syncthreads();
        // ---- the step: the clipped float32 action widened, stepped as a float64 row (act32 == 0) or as the float32 row it is
        double actx = 0, acty = 0;
        if (amine) {
            const float2 c = act[a];
            actx = (double)c.x; acty = (double)c.y;
            if (P.actions) reinterpret_cast<double2 *>(P.actions)[((size_t)env * S + t) * N_AGENTS + a] = make_double2(actx, acty);
        }
        block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny, P.act32 != 0, true);
        if (traced) {
            if (mine) reinterpret_cast<double2 *>(P.tr_x)[(size_t)t * N_LOCUSTS + j] = make_double2(xj, yj);
            if (amine) reinterpret_cast<double2 *>(P.tr_xa)[(size_t)t * N_AGENTS + a] = L.p[0][N_LOCUSTS + a];
        }
        // Every lane reads the same reward behind block_step's closing barrier, but a value from LDS is per-lane to the compiler: a
        // loop that ends on it is laid out as a divergent one (lane 0, whose branch below holds the same test, was sent through the
        // next step alone, its wave one set of barriers ahead of the others).  readfirstlane makes the end of the episode a scalar branch.
        const double r = L.rew[0];
        const bool fin = __builtin_amdgcn_readfirstlane(((r >= 0) || (t + 1 >= t_limit)) ? 1 : 0) != 0;      // multiagent.py:44 + TimeLimit, as the step decides `done`
        if (tid == 0) P.rewards[(size_t)env * S + t] = r;
        if (fin || t + 1 >= n_end) {                           // no exit from inside a per-lane branch
            if (tid == 0) {
                P.length[env] = t + 1;
                P.finished[env] = fin ? 1 : 0;
            }
            break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the eval buffers leave the handle's allocation list with the net (the handle frees what is left on it)
static void fe_release(grl_fieldnet *net) {
    if (!net->ro || !grl_handle_alive(net->h)) return;
    FieldEval &v = net->ro->ev;
    void *all[] = {v.rewards, v.actions, v.length, v.finished, v.tr_mu, v.tr_sigma, v.tr_value, v.tr_raw, v.tr_lb, v.tr_ab, v.tr_pos, v.tr_x, v.tr_xa};
    std::vector<void *> &list = net->h->allocs;
    for (void *p : all) {
        if (!p) continue;
        auto it = std::find(list.begin(), list.end(), p);
        if (it != list.end()) list.erase(it);
        (void)hipFree(p);
    }
    v = FieldEval();
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_fieldnet_eval(grl_fieldnet *net, int32_t max_steps, int32_t greedy, int32_t rows32, int32_t keep_actions, int32_t trace_env) {
    const char *fn = "grl_fieldnet_eval";
    if (!net) return GRL_E_INVALID;
    if (!net->ro) return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": the net is not bound to its handle (grl_fieldnet_rollout_bind first)");
    grl_handle *h = net->h;
    int rc = fr_check(net, fn);
    if (rc) return rc;
    if ((rc = episode_check_steps(h, fn, max_steps)) || (rc = episode_check_trace_env(h, fn, trace_env)) || (rc = episode_check_idle(h, fn)))
        return paac_fail(net, rc, h->err);
    const size_t E = (size_t)h->E, steps = E * max_steps, act = keep_actions ? steps : 0, trace = trace_env >= 0 ? (size_t)max_steps : 0;
    const size_t largest = std::max(std::max(steps, act * N_AGENTS * 2), trace * N_LOCUSTS * 2);
    if (largest > (size_t)INT32_MAX)
        return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": an output of " + std::to_string(largest) +
                                                 " elements does not fit in int32 (fewer envs or steps per call)");
    if ((rc = fr_prepare(net, fn))) return rc;
    FieldRollout *r = net->ro;
    const size_t lds = FE_HEAD_BYTES + r->lds_bytes;
    if (lds > FR_LDS_BYTES)
        return paac_fail(net, GRL_E_STATE, std::string(fn) + ": an env of this geometry needs " + std::to_string(lds) + " bytes of LDS, more than the " +
                                               std::to_string(FR_LDS_BYTES) + " a workgroup has");
    FieldEval &v = r->ev;
    v.max_steps = 0;
    if ((rc = episode_reserve(h, v.cap_steps, steps, {buf(v.rewards)})) || (rc = episode_reserve(h, v.cap_envs, E, {buf(v.length), buf(v.finished)})) ||
        (rc = episode_reserve(h, v.cap_act, act, {buf(v.actions, N_AGENTS * 2)})) ||
        (rc = episode_reserve(h, v.cap_trace, trace,
                              {buf(v.tr_mu, N_AGENTS * 2), buf(v.tr_sigma, N_AGENTS * 2), buf(v.tr_value), buf(v.tr_raw, N_AGENTS * 2), buf(v.tr_lb, N_LOCUSTS * 2),
                               buf(v.tr_ab, N_AGENTS * 2), buf(v.tr_pos, N_AGENTS * 2), buf(v.tr_x, N_LOCUSTS * 2), buf(v.tr_xa, N_AGENTS * 2)})))
        return paac_fail(net, rc, h->err);
    hipStream_t st = h->stream;
    PAAC_HIP(net, hipMemsetAsync(v.rewards, 0, steps * 8, st));      // rows are defined up to the env's length; the rest reads as zero
    if (act) PAAC_HIP(net, hipMemsetAsync(v.actions, 0, act * N_AGENTS * 2 * 8, st));
    if (trace) {
        struct { void *p; size_t bytes; } rows[] = {{v.tr_mu, 80}, {v.tr_sigma, 80}, {v.tr_value, 4}, {v.tr_raw, 80}, {v.tr_lb, 160}, {v.tr_ab, 20},
                                                    {v.tr_pos, 20}, {v.tr_x, 1280}, {v.tr_xa, 160}};
        for (const auto &e : rows) PAAC_HIP(net, hipMemsetAsync(e.p, 0, trace * e.bytes, st));
    }
    FieldEvalArgs P{};
    swarm_start_state(h, P);
    P.P = net->params; P.hv = fr_head_view(net); P.o = net->off;
    P.G = net->cfg.height; P.F = net->F; P.L = net->L; P.P2 = net->P2; P.HWA = net->HWA; P.D0 = net->D0; P.m0n = r->m0n; P.m1n = r->m1n;
    P.scale = net->cfg.scale;
    P.seed = h->cfg.seed; P.env_off = (uint32_t)h->cfg.env_id_offset; P.counter = (uint32_t)net->act_counter;      // the rollout's key; not advanced
    P.max_steps = max_steps; P.limit = h->cfg.max_episode_steps; P.trace_env = trace_env; P.greedy = greedy ? 1 : 0; P.act32 = rows32 ? 1 : 0;
    P.rewards = v.rewards; P.length = v.length; P.finished = v.finished; P.actions = act ? v.actions : nullptr;
    P.tr_mu = v.tr_mu; P.tr_sigma = v.tr_sigma; P.tr_value = v.tr_value; P.tr_raw = v.tr_raw;
    P.tr_lb = v.tr_lb; P.tr_ab = v.tr_ab; P.tr_pos = v.tr_pos; P.tr_x = v.tr_x; P.tr_xa = v.tr_xa;
    hipError_t attr = hipSuccess;
    rc = episode_launch(h, [&] {      // the math mode selects block_step, never the net's own statements
        swarm_math_dispatch(h, [&](auto M) {
            auto *kernel = field_eval_kernel<decltype(M)::value>;
            if (lds > 48 * 1024) attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (attr == hipSuccess) hipLaunchKernelGGL(kernel, dim3((unsigned)E), dim3(SWARM_TPB), lds, st, P);
        });
    });
    PAAC_HIP(net, attr);
    if (rc) return paac_fail(net, rc, h->err);
    v.max_steps = max_steps; v.trace_env = trace_env; v.keep_actions = keep_actions ? 1 : 0;
    return GRL_OK;
}

int grl_fieldnet_read_eval(grl_fieldnet *net, const char *which, void *host, size_t bytes) {
    if (!net) return GRL_E_INVALID;
    grl_handle *h = net->h;
    static const FieldEval none;
    const FieldEval &v = net->ro ? net->ro->ev : none;
    const size_t E = (size_t)h->E, S = (size_t)v.max_steps;
    const char *untraced = v.trace_env < 0 ? "the last evaluation traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"rewards", v.rewards, E * S * 8}, {"length", v.length, E * 4}, {"finished", v.finished, E},
        {"actions", v.actions, E * S * N_AGENTS * 2 * 8, v.keep_actions ? nullptr : "the last evaluation kept no actions (keep_actions was 0)"},
        {"trace_mu", v.tr_mu, S * 80, untraced}, {"trace_sigma", v.tr_sigma, S * 80, untraced}, {"trace_value", v.tr_value, S * 4, untraced},
        {"trace_raw", v.tr_raw, S * 80, untraced}, {"trace_locust_bins", v.tr_lb, S * 160, untraced}, {"trace_agent_bins", v.tr_ab, S * 20, untraced},
        {"trace_positions", v.tr_pos, S * 20, untraced}, {"trace_x", v.tr_x, S * 1280, untraced}, {"trace_xa", v.tr_xa, S * 160, untraced}};
    const int rc = episode_read(h, "grl_fieldnet_read_eval", GRL_ENV_SWARM, "Swarm", v.max_steps != 0, "grl_fieldnet_eval", outs, nullptr, which, host, bytes);
    return rc ? paac_fail(net, rc, h->err) : GRL_OK;
}

}  // extern "C"
