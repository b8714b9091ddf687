// Greedy evaluation of the A3C Gaussian agent: whole episodes of every env of the handle in ONE launch (PolicyMonitor.eval_once,
// fed_gym/agents/a3c/policy_monitor.py:42-96, for every env at once).  Included by net_gauss.hip inside namespace grl.
//
// A workgroup of 4 waves keeps its 64 envs for the whole episode.  Per step: the trunk and the mu tower (the sigma and value
// towers are not evaluated), the greedy action, the env step of its 64 envs, the window shift, the float64 reward sum and the
// optional trace; then a barrier and the next step.  An env that is done masks its lane; the workgroup leaves when none of its envs
// is still playing, or after max_steps.  Workgroups share nothing, so there is no grid-wide barrier and no residency requirement.
//
// Nothing here restates arithmetic: the forward is a3c_trunk / gauss_tower_fwd / gauss_mu, the action gauss_env_action, the env
// step solow_step_env / trade_step_env (flat_env_dev.h), the window a3c_window_restart / a3c_window_step -- the functions the
// per-step rollout path runs, so the two agree bit for bit.  The trunk and the tower are the forward kernel's instantiations
// (LOOP = false: tile loops unrolled): with the backward's (LOOP = true) a GRU step took 12.2 us against 8.0, and TradeAR1's 20 of
// them put the evaluation above the per-step rollout (DESIGN section 3).  0 B of scratch either way.
//
// The window (net->win), the observation and the env state stay in global memory: lane l of wave 0 writes them for env l of the
// group, all four waves read them behind the workgroup barrier (one CU, one vector L1).  The step's mu and action pass through the
// forward's unused dL/dx rows of the LDS.

struct AEvalArgs {
    AArgs a;                            // P, o, n = E, R; states = the handle's processed observation (E,D), win = the net's windows
    float *win;                         // (E,R,D), the same buffer as a.win
    float *act;                         // (E,A) the action each env is stepped with
    int tanh_action, max_steps, trace_steps;
    double *total;                      // (E)
    int32_t *length;                    // (E)
    uint8_t *finished;                  // (E)
    float *tr_states, *tr_mu, *tr_act, *tr_rew, *tr_done;      // (trace_steps, E, ..) or null
};

__device__ __forceinline__ void gauss_eval_env_step(const SolowParams &S, int env, const float *act, float &reward, bool &done) {
    const SolowStepOut o = solow_step_env(S, env, act[0]);
    reward = o.reward; done = o.done;
}
__device__ __forceinline__ void gauss_eval_env_step(const TradeParams &S, int env, const float *act, float &reward, bool &done) {
    const TradeStepOut o = trade_step_env(S, env, act);
    reward = o.reward; done = o.done;
}

constexpr int L_EV_MU = L_HEAD, L_EV_ACT = L_HEAD + AMAXA, L_EV_LIVE = L_HEAD + 2 * AMAXA;
static_assert(L_EV_LIVE < L_HEAD + NX, "the eval rows overflow the dL/dx rows");

template <int D, typename ENV>
__global__ __launch_bounds__(256, 1) void gauss_eval_kernel(AEvalArgs v, ENV S) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *MU = lds + L_EV_MU * LS, *ACT = lds + L_EV_ACT * LS;
    int *live = reinterpret_cast<int *>(lds + L_EV_LIVE * LS);
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    const int sbase = blockIdx.x * 64, s = sbase + lane, n = v.a.n, R = v.a.R;
    const bool mine = wave == 0 && s < n;            // this lane steps env s
    const int ss = s < n ? s : n - 1;                // lanes past n stay inside their own group's rows
    float *w = v.win + (size_t)ss * R * D;
    const float *obs = v.a.states + (size_t)ss * D;
    float *ea = v.act + (size_t)ss * A;
    bool active = mine;
    double total = 0.0;
    int len = 0, k = 0;
    if (mine) a3c_window_restart(w, R, D, obs);      // history = [state] (policy_monitor.py:63-65)
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < v.max_steps; ++step) {
        a3c_trunk<D, D, false>(v.a, lds, sbase, nullptr);
        gauss_tower_fwd<D, false>(v.a, lds, 0);
        if (wave < A) {
            const float m = gauss_mu(O[wave * LS + lane]);
            MU[wave * LS + lane] = m;
            ACT[wave * LS + lane] = gauss_env_action(m, v.tanh_action);
        }
        __syncthreads();
        if (wave == 0) {
            if (active) {
                const bool tr = step < v.trace_steps;
                const size_t row = (size_t)step * n + s;
                for (int i = 0; i < A; ++i) ea[i] = ACT[i * LS + lane];
                if (tr) {
                    for (int i = 0; i < D; ++i) v.tr_states[row * D + i] = obs[i];
                    for (int i = 0; i < A; ++i) {
                        v.tr_mu[row * A + i] = MU[i * LS + lane];
                        v.tr_act[row * A + i] = ACT[i * LS + lane];
                    }
                }
                float reward;
                bool done;
                gauss_eval_env_step(S, s, ea, reward, done);
                total += (double)reward;              // total_reward += reward (policy_monitor.py:80)
                ++len;
                k = a3c_window_step(w, R, D, k, done, obs);
                if (tr) {
                    v.tr_rew[row] = reward;
                    v.tr_done[row] = done ? 1.0f : 0.0f;
                }
                active = !done;
            }
            const unsigned long long m = __ballot(active);
            if (lane == 0) *live = m != 0ull ? 1 : 0;
        }
        __syncthreads();
        if (*live == 0) break;                        // uniform over the workgroup
    }
    if (mine) {
        v.total[s] = total;
        v.length[s] = len;
        v.finished[s] = active ? 0 : 1;
    }
}
