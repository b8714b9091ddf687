// Included by net_flat.hip (inside namespace grl, after net_flat_rollout.inc): evaluation of the flat PAAC policy, whole episodes of
// every env of the handle in ONE launch (SolowPolicyMonitor.eval_once, fed_gym/agents/paac/policy_monitor.py:84-108, for every env
// at once; TradeAR1 under the flat net has no reference counterpart).
//
// The shape is flat_rollout_kernel<G, false>'s: a workgroup of FNT threads keeps G = 16 / 32 / 64 envs for the whole episode, the
// recurrent GRU kernels in registers, the TradeAR1 account in LDS, the argument block in the net's constant-memory slot.  Per step:
// the window length, the three forward calls (the rollout's instantiations), the action, the env step of the group, total += reward
// in float64 and the optional trace.  An env that is done masks its lane: no further env step, no further trace, its TradeAR1 price
// waves idle.  The workgroup leaves when none of its envs still plays, or after max_steps.  Workgroups share nothing: no grid-wide
// barrier, any number of workgroups.
//
// LDS: the forward's rows, the 5 int rows, the float64 account and the live word -- rollout_lds_floats at steps = 0 (the 3 x steps
// reward / value / mask rows of the rollout are gone; RoLds' RW / VL / MK are not touched here), independent of max_steps.
//
// Nothing is restated: ro_enter, ro_trade_trades and the forward are the rollout's functions, the draw / action / window length /
// account / price transition / Solow step are the device functions its stages call (flat_raw_action, flat_env_action,
// ro_window_len, ro_trade_step_body, ro_solow_env_step_body), so the two agree bit for bit up to each env's first done.
//
// Window rule: the rollout's -- min(max(NH,1), rnn) copies of the current state (quirk Q11), the window the policy is trained under
// and the only one flat_forward_fast takes.  The reference monitor feeds the true last-rnn states (DESIGN section 4).

__host__ __device__ inline int eval_lds_floats(int S0, int n_assets, RolloutArgs *map, int *live_off) {
    const int n = rollout_lds_floats(S0, 0, n_assets, map);
    if (live_off) *live_off = n;
    return n + 2;
}

// all waves: the window length for the forward that follows, and the trace of the observation the step is entered with
__device__ __noinline__ int ev_record(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = R.f.n, S0 = R.f.S0;
    const int len = ro_window_len(R, L, lane);
    if (t < R.ev.trace_steps) {
        for (int idx = tid; idx < R.gs * S0; idx += FNT) {
            const int sl = idx / S0, i = idx - sl * S0;
            if (sbase + sl < E && L.DN[sl] == 0) R.ev.states[((size_t)t * E + sbase + sl) * S0 + i] = L.ST[i * LS + sl];
        }
        if (wave == 0 && ro_env(R, sbase, lane) < E && L.DN[lane] == 0) R.ev.nhist[(size_t)t * E + sbase + lane] = L.NH[lane];
    }
    return len;
}

// all waves: the raw action and the env's of the lanes that still play, and the trace of the heads
__device__ __noinline__ void ev_sample(int slot, float *lds, int t, int sbase, uint32_t counter, int alive) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, env = ro_env(R, sbase, lane);
    const int E = R.f.n, A = R.f.A;
    const bool play = env < E && alive != 0, trace = play && t < R.ev.trace_steps;
    if (wave == FNW - 1 && trace) R.ev.val[(size_t)t * E + env] = L.VSL[lane];
    for (int k = wave; k < A; k += FNW) {
        if (!play) continue;
        const float mu = L.MUL[k * LS + lane], sg = L.SGL[k * LS + lane];
        const float r = flat_raw_action(R.greedy, mu, sg, R.seed, (uint32_t)env + R.env_off, counter, k);
        const float ea = flat_env_action(R.env_kind, r);
        L.ACT[k * LS + lane] = ea;
        if (trace) {
            const size_t o = ((size_t)t * E + env) * A + k;
            R.ev.mu[o] = mu; R.ev.sigma[o] = sg; R.ev.raw[o] = r; R.ev.act[o] = ea;
        }
    }
}

// wave 0: the Solow step of the lanes that still play
__device__ __noinline__ StepOut ev_solow_env_step(int slot, float *lds, int t, int sbase, int alive) {
    RO_ARGS(slot);
    return ro_solow_env_step_body<true>(R, lds, t, sbase, alive != 0);
}

// all waves: account and prices of the lanes that still play (wave 0 returns the step's result)
__device__ __noinline__ StepOut ev_trade_step(int slot, float *lds, int t, int sbase, int alive) {
    RO_ARGS(slot);
    return ro_trade_step_body<true>(R, lds, t, sbase, alive != 0);
}

template <int G>
__global__ __launch_bounds__(FNT) void flat_eval_kernel(int slot, int live_off) {
    const RolloutArgs &R = g_ro_args[slot];
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sbase = blockIdx.x * G, max_steps = R.ev.max_steps;
    const int env = lane < G ? sbase + lane : 0x7fffffff;      // = ro_env (R.gs == G)
    const bool valid = env < R.f.n;
    const bool solow = R.env_kind == GRL_ENV_SOLOW;
    const int *DN = reinterpret_cast<int *>(lds + R.row_int * LS) + LS;
    int *LIVE = reinterpret_cast<int *>(lds + live_off);
    RecW w;
    ff_load_recurrent<G>(R.f, w.g, w.c);
    ro_enter(slot, lds, sbase);      // DN = 0: every env of the group plays
    __syncthreads();
    const uint32_t counter0 = *R.counter_base;
    double total = 0.0;
    int len = 0;
#pragma unroll 1
    for (int t = 0; t < max_steps; ++t) {
        const int wl = ev_record(slot, lds, t, sbase);
        const int alive = (valid && DN[lane] == 0) ? 1 : 0;
        flat_forward_fast_call<G, false>(R.slot, lds, sbase, wl, -1, w);      // ends on a barrier
        ev_sample(slot, lds, t, sbase, counter0 + (uint32_t)t, alive);
        __syncthreads();
        StepOut so{0.f, 0};
        if (solow) {
            if (wave == 0) so = ev_solow_env_step(slot, lds, t, sbase, alive);
        } else {
            ro_trade_trades(slot, lds, lane, wave, env, alive != 0);
            __syncthreads();
            so = ev_trade_step(slot, lds, t, sbase, alive);
        }
        if (wave == 0) {
            if (alive) { total += (double)so.reward; ++len; }
            const unsigned long long m = __ballot(alive && !so.done);
            if (lane == 0) *LIVE = m != 0ull ? 1 : 0;
        }
        __syncthreads();
        if (*LIVE == 0) break;      // uniform over the workgroup
    }
    if (wave == 0 && valid) {
        R.ev.total[env] = total;
        R.ev.length[env] = len;
        R.ev.finished[env] = DN[lane] != 0 ? 1 : 0;
    }
}
