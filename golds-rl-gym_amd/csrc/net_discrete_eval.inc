// Greedy evaluation of the A3C discrete savings-grid agent: whole episodes of every env of the handle in ONE launch
// (PolicyMonitor.eval_once, fed_gym/agents/a3c/policy_monitor.py:42-96, for every env at once).  Included by net_discrete.hip inside
// namespace grl.  The shape of gauss_eval_kernel (net_gauss_eval.inc): a workgroup of 4 waves keeps its 64 envs for the whole
// episode; per step the trunk, the probs tower (the value tower is not evaluated), the softmax and the arg-max, the env step of its
// 64 envs, the window shift, the float64 reward sum and the optional trace; then a barrier and the next step.  An env that is done
// masks its lane; the workgroup leaves when none of its envs is still playing, or after max_steps.
//
// Nothing here restates arithmetic: a3c_trunk / disc_probs_fwd / disc_softmax / disc_greedy / disc_grid, solow_step_env
// (flat_env_dev.h) and a3c_window_restart / a3c_window_step are the functions the per-step rollout path runs, the trunk and the
// tower in the forward kernel's instantiation (LOOP = false), so the two agree bit for bit.  The window, the observation and the env
// state stay in global memory: lane l of wave 0 writes them for env l of the group, all four waves read them behind the barrier.

struct DEvalArgs {
    DArgs a;                            // P, o, n = E, R, K; states = the handle's processed observation (E,2), win = the net's windows
    float *win;                         // (E,R,2), the same buffer as a.win
    float *act;                         // (E) the action each env is stepped with
    int max_steps, trace_steps;
    double *total;                      // (E)
    int32_t *length;                    // (E)
    uint8_t *finished;                  // (E)
    float *tr_states, *tr_act, *tr_rew, *tr_done;      // (trace_steps, E, ..) or null
    int32_t *tr_choice;
};

constexpr int L_EV_LIVE = L_LG + DKMAX;      // behind the probabilities
static_assert(L_EV_LIVE < L_DX + NX, "the eval rows overflow the dL/dx rows");

__global__ __launch_bounds__(256, 1) void disc_eval_kernel(DEvalArgs v, SolowParams S) {
    extern __shared__ float lds[];
    float *PR = lds + L_LG * LS;
    int *live = reinterpret_cast<int *>(lds + L_EV_LIVE * LS);
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    const int sbase = blockIdx.x * 64, s = sbase + lane, n = v.a.n, R = v.a.R, K = v.a.K;
    const bool mine = wave == 0 && s < n;            // this lane steps env s
    const int ss = s < n ? s : n - 1;                // lanes past n stay inside their own group's rows
    float *w = v.win + (size_t)ss * R * DD;
    const float *obs = v.a.states + (size_t)ss * DD;
    bool active = mine;
    double total = 0.0;
    int len = 0, k = 0;
    if (mine) a3c_window_restart(w, R, DD, obs);     // history = [state] (policy_monitor.py:63-65)
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < v.max_steps; ++step) {
        a3c_trunk<DD, DD, false>(v.a, lds, sbase, nullptr);
        disc_probs_fwd<false>(v.a, lds);
        if (wave == 0) {
            disc_softmax(PR, K, lane);
            if (active) {
                const int ch = disc_greedy(PR, K, lane);
                const float act = disc_grid(ch, K, v.a.lb, v.a.ub);
                const bool tr = step < v.trace_steps;
                const size_t row = (size_t)step * n + s;
                v.act[s] = act;
                if (tr) {
                    for (int i = 0; i < DD; ++i) v.tr_states[row * DD + i] = obs[i];
                    v.tr_choice[row] = ch;
                    v.tr_act[row] = act;
                }
                const SolowStepOut o = solow_step_env(S, s, act);
                total += (double)o.reward;            // total_reward += reward (policy_monitor.py:80)
                ++len;
                k = a3c_window_step(w, R, DD, k, o.done, obs);
                if (tr) {
                    v.tr_rew[row] = o.reward;
                    v.tr_done[row] = o.done ? 1.0f : 0.0f;
                }
                active = !o.done;
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
