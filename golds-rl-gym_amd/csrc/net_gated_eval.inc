// Greedy evaluation of the Ticker gated trader: whole episodes of every env of the handle in ONE launch.  Included by
// net_gated.hip inside namespace grl.  The reference has no greedy form of this worker (get_action_from_policy ignores
// `stochastic`, worker.py:466-476); the rule is gated_greedy_pick's (DESIGN section 4).
//
// A workgroup of 4 waves keeps its 64 envs for the whole episode.  Per step: the trunk, the class tower and its softmax, the normal
// tower for mu (the value tower is not evaluated and sigma's softplus is not needed), the greedy pick, the env step of its 64 envs,
// the window rule, the float64 reward sum and the optional trace; then a barrier and the next step.  An env that is done masks its
// lane; the workgroup leaves when none of its envs is still playing, or after max_steps.  Workgroups share nothing, so there is no
// grid-wide barrier and no residency requirement.
//
// Nothing here restates arithmetic: the forward is gated_trunk / gated_tower_fwd / softmax3, the action gated_greedy_pick, the env
// step ticker_step_env (ticker_dev.h), the window a3c_window_restart / a3c_window_step -- the functions the per-step rollout
// path runs, so the two agree bit for bit.  The per-step forward is a function of its own (gated_eval_forward, not inlined), for
// the schedule of its GEMM loops; the kernel's 520 B of scratch per lane are that call's argument block (DESIGN section 3).
//
// The window (net->win), the observation and the env state stay in global memory: lane l of wave 0 writes them for env l of the
// group, all four waves read them behind the workgroup barrier (one CU, one vector L1).  The step's probs, mu, choice, fraction and
// the live word pass through the forward's unused dL/dx rows of the LDS.

struct GEvalArgs {
    GArgs a;                            // P, o, n = E, R; states = the handle's processed observation (E,7), win = the net's windows
    float *win;                         // (E,R,4), the same buffer as a.win
    int max_steps, trace_steps;
    double *total;                      // (E)
    int32_t *length;                    // (E)
    uint8_t *finished;                  // (E)
    float *tr_states, *tr_probs, *tr_mu, *tr_act, *tr_rew, *tr_done;      // (trace_steps, E, ..) or null
    int32_t *tr_choices;
};

// probs (6) and mu (6) where the forward kernel keeps them; sigma's 6 rows stay unused
constexpr int L_EV_PR = L_HEAD, L_EV_MU = L_HEAD + 6, L_EV_CH = L_HEAD + 18, L_EV_FR = L_HEAD + 20, L_EV_LIVE = L_HEAD + 22;
static_assert(L_EV_LIVE < L_HEAD + NX, "the eval rows overflow the dL/dx rows");

// One step's forward for the group at sbase: probs and mu into their LDS rows.  Not inlined: inside the kernel's loop over steps the
// compiler schedules the GEMM k-loops for the fewest registers (one weight load in flight); as a function of its own they get the
// forward kernel's schedule (DESIGN section 3).
__device__ __noinline__ void gated_eval_forward(const GArgs &a, float *lds, int sbase) {
    float *O = lds + L_O * LS, *PR = lds + L_EV_PR * LS, *MU = lds + L_EV_MU * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    gated_trunk(a, lds, sbase, nullptr);
    gated_tower_fwd(a, lds, 0);
    if (wave < 2) {     // wave = asset
        float p0, p1, p2;
        softmax3(O[(3 * wave) * LS + lane], O[(3 * wave + 1) * LS + lane], O[(3 * wave + 2) * LS + lane], p0, p1, p2);
        PR[(3 * wave) * LS + lane] = p0; PR[(3 * wave + 1) * LS + lane] = p1; PR[(3 * wave + 2) * LS + lane] = p2;
    }
    __syncthreads();
    gated_tower_fwd(a, lds, 1);
    for (int i = wave; i < 6; i += 4) MU[i * LS + lane] = O[(2 * i) * LS + lane];
    __syncthreads();
}

__global__ __launch_bounds__(256, 1) void gated_eval_kernel(GEvalArgs v, TickerParams K) {
    extern __shared__ float lds[];
    float *PR = lds + L_EV_PR * LS, *MU = lds + L_EV_MU * LS, *FR = lds + L_EV_FR * LS;
    int *CH = reinterpret_cast<int *>(lds + L_EV_CH * LS);
    int *live = reinterpret_cast<int *>(lds + L_EV_LIVE * LS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sbase = blockIdx.x * 64, s = sbase + lane, n = v.a.n, R = v.a.R;
    const bool mine = wave == 0 && s < n;            // this lane steps env s
    const int ss = s < n ? s : n - 1;                // lanes past n stay inside their own group's rows
    float *w = v.win + (size_t)ss * R * GD;
    const float *obs = v.a.states + (size_t)ss * GS0;
    bool active = mine;
    double total = 0.0;
    int len = 0, k = 0;
    constexpr GD_t D{};      // the row width as a constant inside the window rules: this kernel's code as tuned
    if (mine) a3c_window_restart(w, R, D, obs + GTOFF);      // every env's window starts at its current observation
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < v.max_steps; ++step) {
        gated_eval_forward(v.a, lds, sbase);
        if (wave < 2) {
            const int as = wave;
            int ch;
            float raw, frac;
            gated_greedy_pick(PR[(3 * as) * LS + lane], PR[(3 * as + 1) * LS + lane], PR[(3 * as + 2) * LS + lane], MU[(3 * as) * LS + lane],
                              MU[(3 * as + 1) * LS + lane], MU[(3 * as + 2) * LS + lane], ch, raw, frac);
            CH[as * LS + lane] = ch;
            FR[as * LS + lane] = frac;
        }
        __syncthreads();
        if (wave == 0) {
            if (active) {
                const bool tr = step < v.trace_steps;
                const size_t row = (size_t)step * n + s;
                const int c0 = CH[lane], c1 = CH[LS + lane];
                const float4 act = make_float4((float)c0, (float)c1, FR[lane], FR[LS + lane]);
                if (tr) {
                    for (int i = 0; i < GS0; ++i) v.tr_states[row * GS0 + i] = obs[i];
                    for (int i = 0; i < 6; ++i) {
                        v.tr_probs[row * 6 + i] = PR[i * LS + lane];
                        v.tr_mu[row * 6 + i] = MU[i * LS + lane];
                    }
                    v.tr_choices[row * 2] = c0; v.tr_choices[row * 2 + 1] = c1;
                    v.tr_act[row * 4] = act.x; v.tr_act[row * 4 + 1] = act.y; v.tr_act[row * 4 + 2] = act.z; v.tr_act[row * 4 + 3] = act.w;
                }
                const TickerStepOut o = ticker_step_env(K, s, act);
                total += (double)o.reward;
                ++len;
                k = a3c_window_step(w, R, D, k, o.done, obs + GTOFF);
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
