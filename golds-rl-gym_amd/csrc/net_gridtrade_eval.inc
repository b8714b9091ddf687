// Greedy evaluation of the A3C grid trader: whole TradeAR1 episodes of every env of the handle in ONE launch (PolicyMonitor.eval_once,
// fed_gym/agents/a3c/policy_monitor.py:42-96, for every env at once).  Included by net_gridtrade.hip inside namespace grl.  The
// shape of disc_eval_kernel (net_discrete_eval.inc) with the TradeAR1 step and window handling of gauss_eval_kernel
// (net_gauss_eval.inc): a workgroup of 4 waves keeps its 64 envs for the whole episode; per step the trunk, the probs tower (the
// value tower is not evaluated), on waves 0 and 1 the softmax, the arg-max and the grid value of outputs 0 and 1, then on wave 0 the
// env step of its 64 envs, the window shift, the float64 reward sum and the optional trace; then a barrier and the next step.  A
// TradeAR1 episode ends terminally or at the step cap; either way trade_step_env leaves the reset observation behind a done, the
// window restarts there and the env's lane is masked: nothing is bootstrapped in an evaluation, so the rule that differs from Solow
// (no value behind a terminal state) has no part here.  The workgroup leaves when none of its envs is still playing, or after
// max_steps.
//
// Nothing here restates arithmetic: a3c_trunk / grid_probs_fwd / grid_softmax / grid_greedy / grid_value, trade_step_env (flat_env_dev.h)
// and a3c_window_restart / a3c_window_step are the functions the per-step rollout path runs, the trunk and the tower in the forward
// kernel's instantiation (LOOP = false), so the two agree bit for bit.  The window, the observation and the env state stay in global
// memory: lane l of wave 0 writes them for env l of the group, all four waves read them behind the barrier.  The two outputs'
// choices and grid values pass from their waves to wave 0 through the O rows, which the forward uses for the value head only.

// With K = 48 the two outputs fill the dL/dx rows, so nothing fits behind the probabilities: the step's grid values, choices and
// the liveness word live in the O rows, at any K.
constexpr int L_EV_ACT = L_O, L_EV_CH = L_O + GRID_O, L_EV_LIVE = L_O + 2 * GRID_O;
static_assert(L_EV_LIVE < L_O + 16, "the eval rows overflow the O rows");

__global__ __launch_bounds__(256, 1) void gt_eval_kernel(GridEvalArgs v, TradeParams S) {
    extern __shared__ float lds[];
    float *PR = lds + L_LG * LS, *ACT = lds + L_EV_ACT * LS;
    int *CH = reinterpret_cast<int *>(lds + L_EV_CH * LS), *live = reinterpret_cast<int *>(lds + L_EV_LIVE * LS);
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    const int sbase = blockIdx.x * 64, s = sbase + lane, n = v.a.n, R = v.a.R, K = v.a.K;
    const bool mine = wave == 0 && s < n;            // this lane steps env s
    const int ss = s < n ? s : n - 1;                // lanes past n stay inside their own group's rows
    float *w = v.win + (size_t)ss * R * GRID_D;
    const float *obs = v.a.states + (size_t)ss * GRID_D;
    float *ea = v.act + (size_t)ss * GRID_O;
    bool active = mine;
    double total = 0.0;
    int len = 0, k = 0;
    if (mine) a3c_window_restart(w, R, GRID_D, obs);     // history = [state] (policy_monitor.py:63-65)
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < v.max_steps; ++step) {
        a3c_trunk<GRID_D, GRID_D, false>(v.a, lds, sbase, nullptr);
        grid_probs_fwd<false>(v.a, lds);
        if (wave < GRID_O) {                             // wave o: output o of every env of the group
            float *PRo = PR + wave * K * LS;
            grid_softmax(PRo, K, lane);
            const int ch = grid_greedy(PRo, K, lane);
            CH[wave * LS + lane] = ch;
            ACT[wave * LS + lane] = grid_value(ch, K, v.a.lb, v.a.ub);
        }
        __syncthreads();
        if (wave == 0) {
            if (active) {
                const bool tr = step < v.trace_steps;
                const size_t row = (size_t)step * n + s;
                for (int i = 0; i < GRID_O; ++i) ea[i] = ACT[i * LS + lane];
                if (tr) {
                    for (int i = 0; i < GRID_D; ++i) v.tr_states[row * GRID_D + i] = obs[i];
                    for (int i = 0; i < GRID_O; ++i) {
                        v.tr_choice[row * GRID_O + i] = CH[i * LS + lane];
                        v.tr_act[row * GRID_O + i] = ACT[i * LS + lane];
                    }
                }
                const TradeStepOut o = trade_step_env(S, s, ea);
                total += (double)o.reward;            // total_reward += reward (policy_monitor.py:80)
                ++len;
                k = a3c_window_step(w, R, GRID_D, k, o.done, obs);
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
