// Included by net_flat.hip (inside namespace grl, after net_flat_mfma.inc): the flat PAAC actor loop as ONE persistent kernel.
//
// Reference loop: fed_gym/agents/paac/paac.py:119-172 -- T x [predict, a = mu + sigma*N(0,1), transform_actions_for_env, step every
// env (emulator_runner.py:48-65: step, auto-reset, process_state, history window), bookkeeping :142-157], bootstrap value, masked
// n-step returns.  Envs are independent and the parameters do not move during a rollout, so a workgroup can own a group of envs
// (64; 32 or 16 when that still leaves at most one workgroup per CU -- lanes past the group idle, rows keep 64 columns) for all
// T steps with no synchronisation between workgroups: the group's observation, policy outputs, env actions, done flags and the
// T x 64 rewards / values / masks live in LDS, the TradeAR1 account (float64 quantities and prices) too; global memory sees the
// rollout buffers the gradient step reads, and the env state once at the start and once at the end (Solow: its per-env scalars
// stay in global memory, touched by the env's own lane only).  SURVEY section 7 H5: the hipGraph of ~88 dependent launches this
// replaces spent 42 us per dependent stage on 64 of 256 CUs.
//
// Every piece of arithmetic is the code the stand-alone kernels run (flat_forward_fast, solow_step_env, solow_tape_pair,
// returns_column, episodes_account_env; the TradeAR1 step below repeats trade_step_kernel expression by expression), so the rollout
// buffers are bit-identical to the graph path's (GRL_FLAT_ROLLOUT=graph keeps that path for A/B; tests compare the two).

// what flat_eval_kernel (net_flat_eval.inc) leaves behind: per-env results and the optional trace of the first trace_steps steps
struct EvalOut {
    int max_steps, trace_steps;
    double *total;              // (E)
    int32_t *length;            // (E)
    uint8_t *finished;          // (E)
    float *states, *mu, *sigma, *raw, *act, *val, *rew, *done;      // (trace_steps, E, ..)
    int32_t *nhist;
};

struct RolloutArgs {
    FlatArgs f;                 // P, o, n = E, S0, D, T = rnn, A, scale, bound; global outputs unused
    int slot;                   // the same block in g_flat_args (what the forward reads)
    int gs;                     // envs per workgroup: the kernel instance's G
    int steps, env_kind, needs_tape;
    SolowParams so;
    TradeParams tr;
    const float *obs0;          // (E,S0) observation at entry
    float *ro_states, *ro_hist, *ro_act, *ro_val, *ro_rew, *ro_mask, *ro_y, *ro_adv, *ro_boot;
    int32_t *ro_nhist;
    const uint32_t *counter_base;
    uint64_t seed;
    uint32_t env_off;
    float gamma, lam, clip_lo, clip_hi;
    double *ep_total;
    int32_t *ep_len;
    int64_t *ep_steps;
    grl_episode_record *ep_rec;
    int32_t *ep_count;
    int ep_cap;
    // LDS map in rows of LS floats behind the forward's rows (net_flat_fast.inc, which also holds the heads' outputs and the env
    // actions): r/v/m, per-env ints, and (float offset, even) the float64 account rows
    int row_rvm, row_int, off_f64;
    long long *ts;              // stage timestamps of workgroup 0 (grl_fnet_rollout_stage_times), or nullptr
    int *ts_n;
    int greedy;                 // wave-uniform: raw = mu, nothing is drawn (grl_fnet_set_greedy, grl_fnet_eval(.., greedy))
    EvalOut ev;                 // flat_eval_kernel only (net_flat_eval.inc)
    int off_wl;                 // true window only (net_flat_window.inc): float offset of the per-env window rows in LDS, and
    int32_t *wlen;              // (E) the rows the next forward of every env sees, kept between calls
};

__host__ __device__ inline int rollout_lds_floats(int S0, int steps, int n_assets, RolloutArgs *map) {
    int row = ff_rows(S0);
    const int row_rvm = row; row += 3 * steps;
    const int row_int = row; row += 5;
    int off = row * LS;
    off += off & 1;
    if (map) { map->row_rvm = row_rvm; map->row_int = row_int; map->off_f64 = off; }
    return off + (2 * n_assets + 2) * 64 * 2;      // QL, PL: n_assets rows of 64 doubles each; cash, assets: one row each
}

// The stages are calls (their own register allocation); each forms its reference to the argument block from the slot, made
// wave-uniform, so that the block's fields come through scalar loads from constant memory.  Taken by reference into global
// memory the same fields were FLAT loads with a vector address, waited for one by one and re-read after every store
// (ro_trade_account: six dependent round trips to L2 in a stage one wave runs alone).
__constant__ RolloutArgs g_ro_args[kFlatArgSlots];
#define RO_ARGS(slot) const RolloutArgs &R = g_ro_args[__builtin_amdgcn_readfirstlane(slot)]
struct StepOut { float reward; int done; };      // returned in registers (out-pointers go through scratch and a wait)

// LDS views shared by the stages below
struct RoLds {
    float *ST, *MUL, *SGL, *VSL, *ACT, *RW, *VL, *MK;
    int *NH, *DN, *NST, *EPI, *ELP;      // per env: worker history length, done flag of the step, generator counter (next), episode, TimeLimit counter
    double *QL, *PL, *CL, *AL;           // TradeAR1 account: quantities / prices [asset][64], cash / assets [64]
};
__device__ __forceinline__ RoLds ro_lds(const RolloutArgs &R, float *lds) {
    RoLds L;
    L.ST = lds + FF_ST * LS;
    L.MUL = lds + FF_OUT * LS; L.SGL = L.MUL + MAXA * LS; L.VSL = L.SGL + MAXA * LS; L.ACT = L.VSL + LS;
    L.RW = lds + R.row_rvm * LS; L.VL = L.RW + R.steps * LS; L.MK = L.VL + R.steps * LS;
    L.NH = reinterpret_cast<int *>(lds + R.row_int * LS); L.DN = L.NH + LS; L.NST = L.DN + LS; L.EPI = L.NST + LS; L.ELP = L.EPI + LS;
    L.QL = reinterpret_cast<double *>(lds + R.off_f64); L.PL = L.QL + (size_t)R.tr.n * 64; L.CL = L.PL + (size_t)R.tr.n * 64; L.AL = L.CL + 64;
    return L;
}
// the env of a lane: lanes past the group own none (an index no bound check passes)
__device__ __forceinline__ int ro_env(const RolloutArgs &R, int sbase, int lane) { return lane < R.gs ? sbase + lane : 0x7fffffff; }

// TradeAR1Env._step up to the reward / done test (fed_env.py:300-316) in two stages.  (1) all waves, wave w = asset w: the trade
// of that asset -- q_add uses the cash the step was entered with for every asset (fed_env.py:303-307), so the 16 division
// chains are independent; cost and value terms go to LDS (the head rows of the forward are free during the env step).
// (2) wave 0: cost and value summed IN ASSET ORDER (the reference's np.sum over a 16-vector is sequential: n < 8 ... the same
// order trade_step_kernel uses), reward, done, the worker's auto-reset of the account scalars.  Expression by expression as
// trade_step_kernel; serial on one wave this stage was 11 us of a 120 us step.
__device__ __forceinline__ double *ro_trade_terms(float *lds) { return reinterpret_cast<double *>(lds + FF_BIG * LS); }      // [2][MAXA][64]
static_assert((FF_BIG * LS) % 2 == 0 && 2 * MAXA * 64 * 2 <= 7 * FH * LS, "the trade terms fit the forward's head rows, 8-byte aligned");

__device__ __noinline__ void ro_trade_trades(int slot, float *lds, int lane, int wave, int env, bool valid) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const TradeParams &Tr = R.tr;
    const int n_as = Tr.n;
    double *COST = ro_trade_terms(lds), *VAL = COST + MAXA * 64;
    for (int as = wave; as < n_as; as += FNW) {
        if (!valid) continue;
        const float actf = L.ACT[as * LS + lane];
        if (!(actf >= -1.0f && actf <= 1.0f)) atomicAdd(Tr.err_flag, 1);      // action_space.contains (fed_env.py:301)
        const double act = (double)actf, cash = L.CL[lane];
        const double p = L.PL[as * 64 + lane];
        double q = L.QL[as * 64 + lane];
        const double q_add = act > 0.0 ? (act / (double)n_as) * cash / p : act * q;
        q += q_add;
        COST[as * 64 + lane] = q_add * p;
        VAL[as * 64 + lane] = q * p;
        L.QL[as * 64 + lane] = q;
    }
}

// nst_next: the generator counter after this step; the caller stores it (the price waves still read the old one, see ro_trade_step)
__device__ __forceinline__ StepOut ro_trade_account(const RolloutArgs &R, float *lds, int lane, int env, bool valid, int &nst_next) {
    const RoLds L = ro_lds(R, lds);
    const TradeParams &Tr = R.tr;
    const int n_as = Tr.n;
    const double *COST = ro_trade_terms(lds), *VAL = COST + MAXA * 64;
    float reward = 0.f;
    bool done = false;
    if (valid) {
        double cash = L.CL[lane];
        const double assets_old = L.AL[lane];
        double cost = 0.0, value = 0.0;
        for (int as = 0; as < n_as; ++as) {
            cost += COST[as * 64 + lane];
            value += VAL[as * 64 + lane];
        }
        cash = cash + (-cost);
        const double assets_new = cash + value;
        const bool own_done = assets_new < 1.0;                          // MIN_CASH (fed_env.py:272,313)
        reward = (float)(log(assets_new + 1e-4) - log(assets_old + 1e-4));
        const int el = L.ELP[lane] + 1;
        done = own_done || (Tr.max_steps > 0 && el >= Tr.max_steps);
        nst_next = L.NST[lane] + 1;
        if (done) {      // auto-reset (emulator_runner.py:50-52) -> TradeAR1Env._reset (fed_env.py:323-330)
            cash = Tr.start;
            L.AL[lane] = Tr.start; L.ELP[lane] = 0; L.EPI[lane] = L.EPI[lane] + 1;
            L.NH[lane] = 1;
        } else {
            L.AL[lane] = assets_new; L.ELP[lane] = el;
            const int nn = L.NH[lane] + 1;
            L.NH[lane] = nn > Tr.rnn + 1 ? Tr.rnn + 1 : nn;             // list trimmed to rnn+1 (emulator_runner.py:61)
        }
        L.CL[lane] = cash;
        L.ST[lane] = trade_proc(0, cash);
        Tr.reward[env] = reward;
        Tr.done[env] = done ? 1 : 0;
    }
    return StepOut{reward, done ? 1 : 0};
}

// wave 0: SolowEnv._step + auto-reset of the lane's env (state in global memory, the env's own lane only)
__device__ __forceinline__ StepOut ro_solow_step(const RolloutArgs &R, float *lds, int lane, int env, bool valid) {
    const RoLds L = ro_lds(R, lds);
    float reward = 0.f;
    bool done = false;
    if (valid) {
        const SolowStepOut o = solow_step_env(R.so, env, L.ACT[lane]);
        reward = o.reward; done = o.done;
        L.ST[lane] = o.k / 100.0f;        // SolowStateProcessor (state_processors.py:69-71), as solow_write_obs
        L.ST[LS + lane] = o.z;
        L.NH[lane] = o.nh;
        L.EPI[lane] = done ? R.so.episode[env] : 0;
    }
    return StepOut{reward, done ? 1 : 0};
}

// all waves: es ~ N(0, sigma)^T for the envs of the group that were reset in this step (fed_env.py:248)
__device__ __noinline__ void ro_solow_tapes(int slot, float *lds, unsigned long long mask, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    for (unsigned long long rest = mask; rest; rest &= rest - 1) {
        const int sl = __ffsll((long long)rest) - 1;
        for (int pr = threadIdx.x; pr < R.so.T / 2; pr += FNT) solow_tape_pair(R.so, sbase + sl, L.EPI[sl], pr);
    }
}

// wave 0: bootstrap value and the masked n-step returns / GAE of the lane's column (paac.py:159-172, 177)
__device__ __noinline__ void ro_returns(int slot, float *lds, int lane, int env) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const float boot = L.VSL[lane];
    R.ro_boot[env] = boot;
    returns_column(L.RW + lane, L.VL + lane, L.MK + lane, LS, boot, R.steps, R.gamma, R.lam, R.f.scale, R.clip_lo, R.clip_hi,
                   R.ro_y + env, R.ro_adv + env, (size_t)R.f.n);
}

// the window's true_length of the lane's env (a3c/estimators.py:11-15) for the forward that follows
__device__ __forceinline__ int ro_window_len(const RolloutArgs &R, const RoLds &L, int lane) {
    const int D = R.f.D, Rn = R.f.T;
    int nh = L.NH[lane];
    nh = nh < 1 ? 1 : nh;
    const int nrows = nh < Rn ? nh : Rn;      // min(max(n,1), rnn) copies of the current state (quirk Q11)
    float m = 0.f;
    for (int i = 0; i < D; ++i) m = fmaxf(m, fabsf(L.ST[i * LS + lane]));
    return m > 0.f ? nrows : 0;
}

// all waves: states[t] = shared_states, histories[t] = shared_histories (paac.py:132-133), and the window's true_length
__device__ __noinline__ int ro_record(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = R.f.n, S0 = R.f.S0, Rn = R.f.T;
    const int len = ro_window_len(R, L, lane);
    if (t < R.steps) {
        for (int idx = tid; idx < R.gs * S0; idx += FNT) {
            const int sl = idx / S0, i = idx - sl * S0;
            if (sbase + sl < E) R.ro_states[((size_t)t * E + sbase + sl) * S0 + i] = L.ST[i * LS + sl];
        }
        if (R.env_kind == GRL_ENV_SOLOW) {
            for (int idx = tid; idx < R.gs * Rn * 2; idx += FNT) {
                const int sl = idx / (Rn * 2), rem = idx - sl * (Rn * 2), rr = rem >> 1, c = rem & 1;
                int nn = L.NH[sl]; nn = nn < 1 ? 1 : nn; nn = nn < Rn ? nn : Rn;
                if (sbase + sl < E) R.ro_hist[((size_t)t * E + sbase + sl) * Rn * 2 + rem] = rr < nn ? L.ST[c * LS + sl] : 0.f;
            }
        }
        if (wave == 0 && ro_env(R, sbase, lane) < E) R.ro_nhist[(size_t)t * E + sbase + lane] = L.NH[lane];
    }
    return len;
}

// a = mu + sigma * N(0,1) (paac.py:36) in double, from the stream of (env, step counter, action pair); greedy: a = mu by selection
__device__ __forceinline__ float flat_raw_action(int greedy, float mu, float sigma, uint64_t seed, uint32_t env_id, uint32_t counter, int k) {
    if (greedy) return mu;
    double e0, e1;
    normal_pair(rng_block(seed, env_id, counter, RS_FLAT_ACTION, k >> 1), e0, e1);
    return (float)((double)mu + (double)sigma * ((k & 1) ? e1 : e0));
}
// transform_actions_for_env: the stable sigmoid (SolowRunner, emulator_runner.py:77-79) / tanh (TradeAR1, a3c/worker.py:440-442)
__device__ __forceinline__ float flat_env_action(int env_kind, float r) {
    if (env_kind == GRL_ENV_SOLOW) {
        const float z = expf(-fabsf(r));
        return r >= 0.f ? 1.0f / (1.0f + z) : z / (1.0f + z);
    }
    return tanhf(r);
}

// all waves: values[t]; the raw action and the env's
__device__ __noinline__ void ro_sample(int slot, float *lds, int t, int sbase, uint32_t counter) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, env = ro_env(R, sbase, lane);
    const int E = R.f.n, A = R.f.A;
    const bool valid = env < E;
    if (wave == FNW - 1) {
        const float v = L.VSL[lane];
        L.VL[t * LS + lane] = v;
        if (valid) R.ro_val[(size_t)t * E + env] = v;
    }
    for (int k = wave; k < A; k += FNW) {
        const float r = flat_raw_action(R.greedy, L.MUL[k * LS + lane], L.SGL[k * LS + lane], R.seed, (uint32_t)env + R.env_off, counter, k);
        if (valid) R.ro_act[((size_t)t * E + env) * A + k] = r;
        L.ACT[k * LS + lane] = flat_env_action(R.env_kind, r);
    }
}

// wave 0: R6, rewards / masks of step t from the step's result.  EVAL (flat_eval_kernel): no rollout rows and no episode records --
// the done flag of a lane that played this step (it stays set: the lane is masked from then on) and the step's trace
template <bool EVAL>
__device__ __forceinline__ void ro_bookkeeping(const RolloutArgs &R, float *lds, int t, int lane, int env, bool valid, bool solow, StepOut so) {
    const RoLds L = ro_lds(R, lds);
    const int E = R.f.n;
    const float reward = so.reward;
    const int dn = so.done;
    const bool done = dn != 0;
    if constexpr (EVAL) {
        if (valid) {
            L.DN[lane] = dn;
            if (t < R.ev.trace_steps) { R.ev.rew[(size_t)t * E + env] = reward; R.ev.done[(size_t)t * E + env] = (float)dn; }
        }
    } else {
        L.DN[lane] = dn;
        if (R.ep_total) episodes_account_env(valid, env, reward, done, R.ep_total, R.ep_len, R.ep_steps, R.ep_rec, R.ep_count, R.ep_cap);
        L.RW[t * LS + lane] = reward;
        const float mk = 1.0f - (float)dn;      // episodes_over_masks (paac.py:140)
        L.MK[t * LS + lane] = mk;
        if (valid) { R.ro_rew[(size_t)t * E + env] = reward; R.ro_mask[(size_t)t * E + env] = mk; }
        if (t == R.steps - 1) compact_done(done, env, solow ? R.so.done_list : R.tr.done_list, solow ? R.so.done_count : R.tr.done_count);
    }
}

// wave 0: the Solow step of the group's envs (alive: the lane's env still plays; the rollout's always do)
template <bool EVAL>
__device__ __forceinline__ StepOut ro_solow_env_step_body(const RolloutArgs &R, float *lds, int t, int sbase, bool alive) {
    const int lane = threadIdx.x & 63, env = ro_env(R, sbase, lane);
    const bool valid = env < R.f.n && alive;
    const StepOut so = ro_solow_step(R, lds, lane, env, valid);
    ro_bookkeeping<EVAL>(R, lds, t, lane, env, valid, true, so);
    return so;
}
__device__ __noinline__ void ro_solow_env_step(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    ro_solow_env_step_body<false>(R, lds, t, sbase, true);
}

// all waves: the rest of TradeAR1Env._step behind the trades, as ONE stage of two halves around a barrier.  Wave 0 settles the
// account (reward, done, auto-reset); at the same time waves 8.. compute _price_transition (fed_env.py:296-298) for one pair of
// assets each -- the float64 Box-Muller pair, pow and exp, and the three logarithms of the observation -- which depends on the
// account only through `done`: after the barrier they either commit what they hold or write the reset observation.  (As two stages
// the price waves idled for the account's 3 us and the account's wave for the prices' 9.)  The generator counter of the step is
// read by the price waves before the barrier and advanced by wave 0 after it.
static_assert(MAXA <= 16, "one pair of assets per wave 8..15");
template <bool EVAL>
__device__ __forceinline__ StepOut ro_trade_step_body(const RolloutArgs &R, float *lds, int t, int sbase, bool alive) {
    const RoLds L = ro_lds(R, lds);
    const TradeParams &Tr = R.tr;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), env = ro_env(R, sbase, lane);
    const bool valid = env < R.f.n && alive;
    const int n_as = Tr.n, E = Tr.E, pairs = (n_as + 1) / 2;
    const int j = wave - 8, as0 = 2 * j;
    const bool price_wave = j >= 0 && j < pairs && valid;
    int nst_next = 0;
    StepOut so{0.f, 0};
    double pn[2] = {0.0, 0.0};
    float oq[2] = {0.f, 0.f}, op[2] = {0.f, 0.f};
    if (wave == 0) {
        so = ro_trade_account(R, lds, lane, env, valid, nst_next);
        ro_bookkeeping<EVAL>(R, lds, t, lane, env, valid, false, so);
    } else if (price_wave) {
        double z[2];
        if (Tr.flags & GRL_F_INJECT_NOISE) {
            z[0] = Tr.normals[(size_t)as0 * E + env];
            z[1] = as0 + 1 < n_as ? Tr.normals[(size_t)(as0 + 1) * E + env] : 0.0;
        } else {
            const uint32_t st = (uint32_t)L.NST[lane];      // the counter this step was entered with
            normal_pair(rng_block(Tr.seed, (uint32_t)env + Tr.env_off, 0u, RS_TRADE_PRICE, st * pairs + j), z[0], z[1]);
        }
        for (int k = 0; k < 2 && as0 + k < n_as; ++k) {
            const int ak = as0 + k;
            pn[k] = pow(L.PL[ak * 64 + lane], 0.9) * exp(Tr.std_e * z[k]);
            oq[k] = trade_proc(1, L.QL[ak * 64 + lane]);
            op[k] = trade_proc(1, pn[k]);
        }
    }
    __syncthreads();
    if (wave == 0) {
        if (valid) L.NST[lane] = nst_next;
    } else if (price_wave) {
        const bool reset = L.DN[lane] != 0;
        for (int k = 0; k < 2 && as0 + k < n_as; ++k) {
            const int ak = as0 + k;
            if (reset) {
                L.QL[ak * 64 + lane] = 0.0; L.PL[ak * 64 + lane] = 1.0;
                L.ST[(1 + ak) * LS + lane] = trade_proc(1, 0.0);
                L.ST[(1 + n_as + ak) * LS + lane] = trade_proc(1, 1.0);
            } else {
                L.PL[ak * 64 + lane] = pn[k];
                L.ST[(1 + ak) * LS + lane] = oq[k];
                L.ST[(1 + n_as + ak) * LS + lane] = op[k];
            }
        }
    }
    return so;
}
__device__ __noinline__ void ro_trade_step(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    ro_trade_step_body<false>(R, lds, t, sbase, true);
}

// all waves: the group's observation and per-env scalars into LDS
__device__ __noinline__ void ro_enter(int slot, float *lds, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, env = ro_env(R, sbase, lane);
    const int E = R.f.n, S0 = R.f.S0;
    const bool valid = env < E, solow = R.env_kind == GRL_ENV_SOLOW;
    const TradeParams &Tr = R.tr;
    for (int idx = tid; idx < 64 * S0; idx += FNT) {
        const int sl = idx / S0, i = idx - sl * S0;
        L.ST[i * LS + sl] = (sl < R.gs && sbase + sl < E) ? R.obs0[(size_t)(sbase + sl) * S0 + i] : 0.f;
    }
    if (wave == 0) {
        L.NH[lane] = valid ? (solow ? R.so.nhist[env] : Tr.nhist[env]) : 1;
        L.DN[lane] = 0; L.NST[lane] = 0; L.EPI[lane] = 0; L.ELP[lane] = 0;
        if (!solow) {
            L.CL[lane] = valid ? Tr.cash[env] : Tr.start; L.AL[lane] = valid ? Tr.assets[env] : Tr.start;
            if (valid) { L.ELP[lane] = Tr.elapsed[env]; L.EPI[lane] = Tr.episode[env]; L.NST[lane] = (int)Tr.nstep[env]; }
        }
    }
    if (!solow)
        for (int as = wave; as < Tr.n; as += FNW) {
            L.QL[as * 64 + lane] = valid ? Tr.q[(size_t)as * E + env] : 0.0;
            L.PL[as * 64 + lane] = valid ? Tr.p[(size_t)as * E + env] : 1.0;
        }
}

// all waves: the TradeAR1 account and observation back to the handle (Solow kept its state in global memory all along)
__device__ __noinline__ void ro_leave_trade(int slot, float *lds, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, env = ro_env(R, sbase, lane);
    const int E = R.f.n, S0 = R.f.S0;
    const bool valid = env < E;
    const TradeParams &Tr = R.tr;
    const int n_as = Tr.n;
    if (wave == 0 && valid) {
        Tr.cash[env] = L.CL[lane]; Tr.assets[env] = L.AL[lane]; Tr.elapsed[env] = L.ELP[lane]; Tr.episode[env] = L.EPI[lane];
        Tr.nstep[env] = (uint32_t)L.NST[lane]; Tr.nhist[env] = L.NH[lane];
    }
    for (int as = wave; as < n_as; as += FNW)
        if (valid) { Tr.q[(size_t)as * E + env] = L.QL[as * 64 + lane]; Tr.p[(size_t)as * E + env] = L.PL[as * 64 + lane]; }
    for (int idx = tid; idx < R.gs * S0; idx += FNT) {
        const int sl = idx / S0, i = idx - sl * S0;
        if (sbase + sl >= E) continue;
        const size_t o = (size_t)(sbase + sl) * S0 + i;
        Tr.obs[o] = L.ST[i * LS + sl];
        Tr.obs_raw[o] = i == 0 ? (float)L.CL[sl] : (i <= n_as ? (float)L.QL[(i - 1) * 64 + sl] : (float)L.PL[(i - 1 - n_as) * 64 + sl]);
    }
}

// The argument block lives in constant memory (uploaded before the launch, one slot per net): a by-value kernel argument whose
// address escapes is copied into every lane's scratch first (1.3 KB per lane here).
template <int G, bool KEEP>
__global__ __launch_bounds__(FNT) void flat_rollout_kernel(int slot) {
    const RolloutArgs &R = g_ro_args[slot];
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sbase = blockIdx.x * G, steps = R.steps;
    const int env = lane < G ? sbase + lane : 0x7fffffff;      // = ro_env (R.gs == G)
    const bool valid = env < R.f.n;
    const bool solow = R.env_kind == GRL_ENV_SOLOW;
    RecW w;
    ff_load_recurrent<G>(R.f, w.g, w.c);      // the recurrent GRU kernels stay in registers for the whole rollout
    ro_enter(slot, lds, sbase);
    __syncthreads();
    FwdLocal st{};
    st.ts = R.ts; st.ts_n = R.ts_n;
    fwd_stamp(st);
    const uint32_t counter0 = *R.counter_base;
    for (int t = 0; t <= steps; ++t) {
        const int len = ro_record(slot, lds, t, sbase);
        fwd_stamp(st);
        flat_forward_fast_call<G, KEEP>(R.slot, lds, sbase, len, t < steps ? t * R.f.n + sbase : -1, w);      // ends on a barrier
        if (t == steps) break;      // that was the bootstrap forward (paac.py:159-165)
        ro_sample(slot, lds, t, sbase, counter0 + (uint32_t)t);
        __syncthreads();
        fwd_stamp(st);
        if (!solow) {
            ro_trade_trades(slot, lds, lane, wave, env, valid);
            __syncthreads();
        }
        if (solow) {
            if (wave == 0) ro_solow_env_step(slot, lds, t, sbase);
        } else {
            ro_trade_step(slot, lds, t, sbase);
        }
        __syncthreads();
        fwd_stamp(st);
        if (solow) {
            if (R.needs_tape) {
                const int *DN = reinterpret_cast<int *>(lds + R.row_int * LS) + LS;
                const unsigned long long m = __ballot(DN[lane] != 0);
                if (m) {
                    ro_solow_tapes(slot, lds, m, sbase);
                    __syncthreads();
                }
            }
        }
        fwd_stamp(st);
    }
    if (wave == 0 && valid) ro_returns(slot, lds, lane, env);
    fwd_stamp(st);
    if (!solow) ro_leave_trade(slot, lds, sbase);
}
