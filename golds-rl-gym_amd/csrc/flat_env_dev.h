// Device-side pieces of the Solow-v0 / TradeAR1-v0 step shared by the stand-alone step kernels (flat_envs.hip), the persistent
// flat PAAC rollout (net_flat.hip: one workgroup keeps 64 envs for all T steps) and the Gaussian agent's greedy evaluation
// (net_gauss_eval.inc): parameter blocks, the per-env Solow and TradeAR1 steps with the worker's auto-reset, the shock-tape draw,
// the TradeAR1 observation transform.  Reference: fed_gym/envs/fed_env.py:161-334,
// fed_gym/agents/paac/emulator_runner.py:48-65.
#pragma once
#include <type_traits>
#include "common.h"
#include "rng.h"

namespace grl {

// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void compact_done(bool done, int env, int32_t *done_list, int32_t *done_count) {
    unsigned long long m = __ballot(done);
    if (m == 0) return;
    int lane = threadIdx.x & 63;
    int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(done_count, __popcll(m));
    base = __shfl(base, leader);
    if (done) done_list[base + __popcll(m & ((1ull << lane) - 1ull))] = env;
}

// ------------------------------------------------------------------------------------------ Solow
struct SolowParams {
    float *k, *z, *e, *z0, *tape;
    int32_t *tape_pos, *nhist, *elapsed, *episode;
    const float *actions;
    float *reward;
    uint8_t *done;
    float *obs_raw, *obs, *history;
    float *term_obs;      // (E,2) or null: the processed observation an episode ended in, before the auto-reset overwrites it
    int32_t *done_list, *done_count, *err_flag;
    const int32_t *reset_list, *reset_count;
    int E, P, Q, T, rnn, max_steps;
    float rho_z[8], rho_e[8];
    float delta, sigma, kss;
    uint32_t flags, env_off;
    uint64_t seed;
};

// SolowStateProcessor: obs / [100, 1] (state_processors.py:69-71) and the history window as the
// worker builds it (quirk Q11: min(n,rnn) copies of the CURRENT state, zero padded at the end)
__device__ __forceinline__ void solow_write_obs(const SolowParams &S, int env, float k, float zl, int nh) {
    reinterpret_cast<float2 *>(S.obs_raw)[env] = make_float2(k, zl);
    float2 o = make_float2(k / 100.0f, zl);
    reinterpret_cast<float2 *>(S.obs)[env] = o;
    int n = nh < S.rnn ? nh : S.rnn;
    for (int r = 0; r < S.rnn; ++r)
        reinterpret_cast<float2 *>(S.history)[(size_t)env * S.rnn + r] = r < n ? o : make_float2(0.f, 0.f);
}

// SolowEnv._reset without the tape (fed_env.py:242-250): k = k_ss(0.33), e = 0, z ~ N(0, sigma)^p
__device__ __forceinline__ float solow_reset_env(const SolowParams &S, int env) {
    S.k[env] = S.kss;
    for (int i = 0; i < S.Q; ++i) S.e[(size_t)i * S.E + env] = 0.f;
    const bool fixed = S.flags & (GRL_F_RESET_FROM_SNAPSHOT | GRL_F_RESEED_EACH_RESET);
    float zl = 0.f;
    if (S.flags & GRL_F_SOLOW_SS_RESET) {      // SolowSSEnv._reset (fed_env.py:259): self.z = np.array([0.])
        for (int i = 0; i < S.P; ++i) S.z[(size_t)i * S.E + env] = 0.f;
    } else if (fixed && (S.flags & GRL_F_RESET_FROM_SNAPSHOT)) {
        for (int i = 0; i < S.P; ++i) { zl = S.z0[(size_t)i * S.E + env]; S.z[(size_t)i * S.E + env] = zl; }
    } else {
        uint32_t ep = (S.flags & GRL_F_RESEED_EACH_RESET) ? 0u : (uint32_t)S.episode[env];
        for (int i = 0; i < S.P; i += 2) {
            double n0, n1;
            normal_pair(rng_block(S.seed, (uint32_t)env + S.env_off, ep, RS_SOLOW_Z0, i >> 1), n0, n1);
            zl = (float)((double)S.sigma * n0);
            S.z[(size_t)i * S.E + env] = zl;
            if (i + 1 < S.P) { zl = (float)((double)S.sigma * n1); S.z[(size_t)(i + 1) * S.E + env] = zl; }
        }
    }
    S.tape_pos[env] = S.T - 1;
    S.elapsed[env] = 0;
    S.nhist[env] = 1;            // histories[i] = [reset state]  (emulator_runner.py:52)
    S.episode[env] = S.episode[env] + 1;
    return zl;
}

// SolowEnv._step + the worker's auto-reset for ONE env (fed_env.py:201-236, emulator_runner.py:48-65): updates the env's state
// in global memory, writes reward / done / observation / history window, returns what a fused caller keeps in registers.
struct SolowStepOut { float reward, k, z; int nh; bool done; };
__device__ __forceinline__ SolowStepOut solow_step_env(const SolowParams &S, int env, float action) {
    SolowStepOut o;
    float s = fmaxf(1e-3f, action);
    float k = S.k[env];
    float zl = S.z[(size_t)(S.P - 1) * S.E + env];
    float y = expf(zl) * powf(k, 0.33f);
    float kn = (1.0f - S.delta) * k + s * y;
    int pos = S.tape_pos[env];
    float e_t = 0.f;
    if (pos >= 0) e_t = S.tape[(size_t)pos * S.E + env];   // es.pop(): from the end (quirk Q8)
    else atomicAdd(S.err_flag, 1);                          // reference: IndexError, pop from empty list
    S.tape_pos[env] = pos - 1;
    float ar = 0.f, ma = 0.f;
    for (int i = 0; i < S.P; ++i) ar += S.rho_z[i] * S.z[(size_t)i * S.E + env];
    for (int i = 0; i < S.Q; ++i) ma += S.rho_e[i] * S.e[(size_t)i * S.E + env];
    float zn = (ar + ma) + e_t;
    for (int i = 0; i + 1 < S.P; ++i) S.z[(size_t)i * S.E + env] = S.z[(size_t)(i + 1) * S.E + env];
    S.z[(size_t)(S.P - 1) * S.E + env] = zn;
    for (int i = 0; i + 1 < S.Q; ++i) S.e[(size_t)i * S.E + env] = S.e[(size_t)(i + 1) * S.E + env];
    S.e[(size_t)(S.Q - 1) * S.E + env] = e_t;
    S.k[env] = kn;
    o.reward = logf((1.0f - s) * y + 1e-4f);
    S.reward[env] = o.reward;
    int el = S.elapsed[env] + 1;
    o.done = S.max_steps > 0 && el >= S.max_steps;    // Solow itself never ends (fed_env.py:234)
    S.done[env] = o.done ? 1 : 0;
    int nh;
    if (o.done) {   // auto-reset: terminal reward stays, observation is the reset one (quirk Q6)
        if (S.term_obs) reinterpret_cast<float2 *>(S.term_obs)[env] = make_float2(kn / 100.0f, zn);
        zn = solow_reset_env(S, env);
        kn = S.kss;
        nh = 1;
    } else {
        S.elapsed[env] = el;
        nh = S.nhist[env] + 1;
        if (nh > S.rnn + 1) nh = S.rnn + 1;           // list is trimmed to rnn+1 (emulator_runner.py:61)
        S.nhist[env] = nh;
    }
    solow_write_obs(S, env, kn, zn, nh);
    o.k = kn; o.z = zn; o.nh = nh;
    return o;
}

// The arithmetic of solow_step_env on values held in registers, for a caller that keeps an env's whole state there and plays
// several savings rates over one shock path (solow_sweep.hip).  Same operations in the same order as lines of solow_step_env
// above, so the two give the same bits (tests/test_gpu_solow_sweep.py holds them together).
//
// The shock history is kept right-aligned in eight registers: zr[8 - P + i] = z[i], so zr[7] is z[-1] and the shift needs no
// runtime index; rz / re are rho_z / rho_e aligned the same way by the host.  Slots below 8 - P are never read: the sums skip
// them with a uniform branch instead of adding 0 * z terms.
struct SolowShockCoef { float rz[8], re[8]; int P, Q; };

__device__ __forceinline__ float solow_shock_next(const SolowShockCoef &C, float (&zr)[8], float (&er)[8], float e_t) {
    float ar = 0.f, ma = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j >= 8 - C.P) ar += C.rz[j] * zr[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j >= 8 - C.Q) ma += C.re[j] * er[j];
    const float zn = (ar + ma) + e_t;
#pragma unroll
    for (int j = 0; j < 7; ++j) { zr[j] = zr[j + 1]; er[j] = er[j + 1]; }
    zr[7] = zn;
    er[7] = e_t;
    return zn;
}

// one rate's share of the step: ez = expf(z[-1]) is the same for every rate of the env.  Advances k, returns the reward.
__device__ __forceinline__ float solow_capital_step(float ez, float delta, float rate, float &k) {
    const float s = fmaxf(1e-3f, rate);
    const float y = ez * powf(k, 0.33f);
    k = (1.0f - delta) * k + s * y;
    return logf((1.0f - s) * y + 1e-4f);
}

// es = N(0, sigma)^T: pair `pr` of the tape of `env` (fed_env.py:248); episode[env] was already advanced by the reset
__device__ __forceinline__ void solow_tape_pair(const SolowParams &S, int env, int episode_after_reset, int pr) {
    uint32_t ep = (S.flags & GRL_F_RESEED_EACH_RESET) ? 0u : (uint32_t)(episode_after_reset - 1);
    double n0, n1;
    normal_pair(rng_block(S.seed, (uint32_t)env + S.env_off, ep, RS_SOLOW_TAPE, pr), n0, n1);
    S.tape[(size_t)(2 * pr) * S.E + env] = (float)((double)S.sigma * n0);
    S.tape[(size_t)(2 * pr + 1) * S.E + env] = (float)((double)S.sigma * n1);
}

static inline SolowParams solow_params(grl_handle *h) {
    SolowParams S{};
    S.k = h->so.k; S.z = h->so.z; S.e = h->so.e; S.z0 = h->so.z0; S.tape = h->so.tape;
    S.tape_pos = h->so.tape_pos; S.nhist = h->so.nhist; S.elapsed = h->elapsed; S.episode = h->episode;
    S.reward = h->reward; S.done = h->done; S.obs_raw = h->so.obs_raw; S.obs = h->so.obs; S.history = h->so.history;
    S.done_list = h->done_list; S.done_count = h->done_count; S.err_flag = h->err_flag;
    S.E = h->E; S.P = h->so.P; S.Q = h->so.Q; S.T = h->cfg.solow_tape_len; S.rnn = h->cfg.rnn_length;
    S.max_steps = h->cfg.max_episode_steps;
    for (int i = 0; i < 8; ++i) { S.rho_z[i] = h->so.rho_z[i]; S.rho_e[i] = h->so.rho_e[i]; }
    S.delta = (float)h->cfg.solow_delta; S.sigma = (float)h->cfg.solow_sigma;
    S.kss = (float)pow(0.33 / h->cfg.solow_delta, 1.0 / (1.0 - 0.33));   // _k_ss(0.33) (fed_env.py:198-199,243)
    S.flags = h->cfg.flags; S.env_off = (uint32_t)h->cfg.env_id_offset; S.seed = h->cfg.seed;
    return S;
}

// rho_z / rho_e right-aligned, as solow_shock_next reads them
static inline SolowShockCoef solow_shock_coef(const SolowParams &S) {
    SolowShockCoef C{};
    C.P = S.P; C.Q = S.Q;
    for (int i = 0; i < S.P; ++i) C.rz[8 - S.P + i] = S.rho_z[i];
    for (int i = 0; i < S.Q; ++i) C.re[8 - S.Q + i] = S.rho_e[i];
    return C;
}


// ------------------------------------------------------------------------------------------ TradeAR1
struct TradeParams {
    double *cash, *assets, *q, *p;
    const float *normals;
    uint32_t *nstep;
    int32_t *elapsed, *episode, *nhist;
    int rnn;
    const float *actions;
    float *reward;
    uint8_t *done;
    float *obs_raw, *obs;
    int32_t *done_list, *done_count, *err_flag;
    const int32_t *reset_list, *reset_count;
    int E, n, max_steps;
    double std_e;
    double start;                     // TradeAR1Env.starting_balance: cash = assets = start after a reset (fed_env.py:323-326)
    uint32_t flags, env_off;
    uint64_t seed;
};

// TradeWorker.process_state as it behaves (a3c/worker.py:420-431, quirk Q10):
// [log(cash+1e-4), log(q+1)..., log(p+1)...]; evaluated in float64 like the reference, rounded for the float32 net input
__device__ __forceinline__ float trade_proc(int idx, double v) { return (float)(idx == 0 ? log(v + 1e-4) : log(v + 1.0)); }

static inline TradeParams trade_params(grl_handle *h) {
    TradeParams R{};
    R.cash = h->tr.cash; R.assets = h->tr.assets; R.q = h->tr.q; R.p = h->tr.p; R.normals = h->tr.normals;
    R.nstep = h->tr.nstep; R.nhist = h->tr.nhist; R.rnn = h->cfg.rnn_length; R.elapsed = h->elapsed; R.episode = h->episode; R.reward = h->reward; R.done = h->done;
    R.obs_raw = h->tr.obs_raw; R.obs = h->tr.obs; R.done_list = h->done_list; R.done_count = h->done_count;
    R.err_flag = h->err_flag; R.E = h->E; R.n = h->cfg.n_assets; R.max_steps = h->cfg.max_episode_steps;
    R.std_e = h->tr.std_e; R.start = h->tr.start; R.flags = h->cfg.flags; R.env_off = (uint32_t)h->cfg.env_id_offset; R.seed = h->cfg.seed;
    return R;
}

// TradeAR1Env._step + the worker's auto-reset for ONE env (fed_env.py:300-330, emulator_runner.py:48-65); actions: the env's n
// actions.  Updates the env's account in global memory, writes reward / done / observation, returns what a fused caller keeps in
// registers.
struct TradeStepOut { float reward; bool done; };
__device__ __forceinline__ TradeStepOut trade_step_env(const TradeParams &R, int env, const float *actions) {
    TradeStepOut o_;
    const int n = R.n, S = 1 + 2 * n;
    const size_t E = R.E;
    // TradeAR1Env._step (fed_env.py:300-321)
    double cash = R.cash[env];
    const double assets_old = R.assets[env];
    double cost = 0.0, value = 0.0;
    bool bad = false;
    for (int a = 0; a < n; ++a) {
        const float actf = actions[a];
        bad |= !(actf >= -1.0f && actf <= 1.0f);                     // action_space.contains (fed_env.py:301)
        const double act = (double)actf;
        const double p = R.p[a * E + env];
        double q = R.q[a * E + env];
        const double q_add = act > 0.0 ? (act / (double)n) * cash / p : act * q;
        q += q_add;
        cost += q_add * p;
        value += q * p;
        R.q[a * E + env] = q;
    }
    if (bad) atomicAdd(R.err_flag, 1);
    cash = cash + (-cost);
    const double assets = cash + value;
    const bool own_done = assets < 1.0;                              // MIN_CASH (fed_env.py:272,313)
    o_.reward = (float)(log(assets + 1e-4) - log(assets_old + 1e-4));
    R.reward[env] = o_.reward;
    const int el = R.elapsed[env] + 1;
    const bool done = own_done || (R.max_steps > 0 && el >= R.max_steps);
    R.done[env] = done ? 1 : 0;
    const uint32_t st = R.nstep[env];
    R.nstep[env] = st + 1;
    float *oraw = R.obs_raw + (size_t)env * S, *o = R.obs + (size_t)env * S;
    if (done) {   // auto-reset (emulator_runner.py:50-52) -> TradeAR1Env._reset (fed_env.py:323-330)
        cash = R.start;
        R.assets[env] = R.start;
        R.elapsed[env] = 0;
        R.nhist[env] = 1;            // histories[i] = [reset state]  (emulator_runner.py:52)
        R.episode[env] = R.episode[env] + 1;
        for (int a = 0; a < n; ++a) {
            R.q[a * E + env] = 0.0; R.p[a * E + env] = 1.0;
            oraw[1 + a] = 0.f; oraw[1 + n + a] = 1.f;
            o[1 + a] = trade_proc(1, 0.0); o[1 + n + a] = trade_proc(1, 1.0);
        }
    } else {
        R.assets[env] = assets;
        R.elapsed[env] = el;
        {
            const int nh = R.nhist[env] + 1;
            R.nhist[env] = nh > R.rnn + 1 ? R.rnn + 1 : nh;     // list trimmed to rnn+1 (emulator_runner.py:61)
        }
        const int pairs = (n + 1) / 2;
        for (int a = 0; a < n; a += 2) {
            double z[2];
            if (R.flags & GRL_F_INJECT_NOISE) {
                z[0] = R.normals[a * E + env];
                z[1] = a + 1 < n ? R.normals[(a + 1) * E + env] : 0.0;
            } else {
                normal_pair(rng_block(R.seed, (uint32_t)env + R.env_off, 0u, RS_TRADE_PRICE, st * pairs + (a >> 1)), z[0], z[1]);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int ak = a + k;
                if (ak >= n) break;
                // _price_transition: p**rho_p * exp(std_e * N(0,1))  (fed_env.py:296-298)
                const double p = pow(R.p[ak * E + env], 0.9) * exp(R.std_e * z[k]);
                R.p[ak * E + env] = p;
                const double q = R.q[ak * E + env];
                oraw[1 + ak] = (float)q; oraw[1 + n + ak] = (float)p;
                o[1 + ak] = trade_proc(1, q); o[1 + n + ak] = trade_proc(1, p);
            }
        }
    }
    R.cash[env] = cash;
    oraw[0] = (float)cash;
    o[0] = trade_proc(0, cash);
    o_.done = done;
    return o_;
}

// The arithmetic of trade_step_env on values the caller holds (registers, or LDS columns for many assets), for a caller that keeps
// an env's account there and plays several scripted rules over one price path (trade_sweep.hip).  Same operations in the same
// order as the account lines and the price line of trade_step_env above, so the two give the same bits
// (tests/test_gpu_trade_sweep.py holds them together).  The caller walks the assets in order and calls trade_rule_action and
// trade_asset_trade for each, then trade_account_settle once.

// the scripted rule (include/goldsrl_tradesweep.h): clip(bias - gain * (p - 1), -1, 1) in float64, one IEEE operation per line,
// rounded to the float32 action the env is stepped with (trade_rule_action, below its four-number form).
// the four-number rule of the search (include/goldsrl_tradesearch.h): a gain for each side of a reference level `ref`, the side a
// select on the sign of p - ref (d == 0 takes gain_sell; m is 0 either way).  The same one-operation lines; with gain_buy ==
// gain_sell the select has one operand and ref = 1.0 makes the lines trade_rule_action's, which is that call.
__device__ __forceinline__ float trade_rule4_action(double gain_buy, double gain_sell, double bias, double ref, double p) {
    const double d = p - ref;
    const double g = d < 0.0 ? gain_buy : gain_sell;
    const double m = g * d;
    double x = bias - m;
    x = fmin(fmax(x, -1.0), 1.0);
    return (float)x;
}

__device__ __forceinline__ float trade_rule_action(double gain, double bias, double p) { return trade_rule4_action(gain, gain, bias, 1.0, p); }

// one asset's trade: buys are sized from the cash before any purchase of this step; cost and value accumulate in asset order
__device__ __forceinline__ void trade_asset_trade(float actf, int n, double cash, double p, double &q, double &cost, double &value) {
    const double act = (double)actf;
    const double q_add = act > 0.0 ? (act / (double)n) * cash / p : act * q;
    q += q_add;
    cost += q_add * p;
    value += q * p;
}

// the end of the account step: advances cash and assets, returns the reward; depleted = assets < MIN_CASH
__device__ __forceinline__ float trade_account_settle(double &cash, double &assets, double cost, double value, bool &depleted) {
    const double assets_old = assets;
    cash = cash + (-cost);
    assets = cash + value;
    depleted = assets < 1.0;
    return (float)(log(assets + 1e-4) - log(assets_old + 1e-4));
}

// _price_transition on a value: p**rho_p * exp(std_e * N(0,1))
__device__ __forceinline__ double trade_price_next(double p, double std_e, double z) { return pow(p, 0.9) * exp(std_e * z); }

// the two normals of asset pair `pr` at generator step `st` of `env`: the key and counter trade_step_env draws with
__device__ __forceinline__ void trade_price_normals(uint64_t seed, uint32_t env_id, uint32_t st, int pairs, int pr, double &z0, double &z1) {
    normal_pair(rng_block(seed, env_id, 0u, RS_TRADE_PRICE, st * (uint32_t)pairs + (uint32_t)pr), z0, z1);
}

// ---- the asset tiers of the whole-episode TradeAR1 kernels (trade_sweep.hip, trade_foresight.hip): up to 16 assets live in
// registers, in compile-time tiers NT = 2 / 4 / 8 / 16; from 17 to 64 (NT = 0) in LDS columns or global memory.
// f(a) for a = 0 .. n-1: unrolled to NT slots under a uniform guard (registers), or a plain loop (NT = 0)
template <int NT, class F>
__device__ __forceinline__ void trade_for(int n, F f) {
    if constexpr (NT > 0) {
#pragma unroll
        for (int a = 0; a < NT; ++a)
            if (a < n) f(a);
    } else {
        for (int a = 0; a < n; ++a) f(a);
    }
}

// _price_transition of every asset of `env` by the draws of step index t: row t of the tape (t, n, E), or the generator at
// st0 + t.  get(a) reads, put(a, p) writes asset a's price; pairs = (n + 1) / 2.  trade_path_kernel keeps a written-out twin.
template <int NT, class G, class P>
__device__ __forceinline__ void trade_prices_step(const TradeParams &R, const float *__restrict__ tape, int env, uint32_t st0, int t, int pairs, G get, P put) {
    const size_t E = R.E;
    const int n = R.n;
    const uint32_t st = st0 + (uint32_t)t;
    trade_for<(NT + 1) / 2>(pairs, [&](int k) {
        const int a = 2 * k;
        double z0, z1 = 0.0;
        if (tape) {
            z0 = (double)tape[((size_t)t * n + a) * E + env];
            if (a + 1 < n) z1 = (double)tape[((size_t)t * n + a + 1) * E + env];
        } else {
            trade_price_normals(R.seed, (uint32_t)env + R.env_off, st, pairs, k, z0, z1);   // an odd n discards the last z1
        }
        put(a, trade_price_next(get(a), R.std_e, z0));
        if (a + 1 < n) put(a + 1, trade_price_next(get(a + 1), R.std_e, z1));       // NT is even: slot a + 1 exists
    });
}

constexpr int TRADE_LDS_BYTES = 160 * 1024;      // of a CU

// ---- host half of the same two launches, no device code from here on.  The tier of n assets: pick(std::integral_constant<int,
// NT>) takes the caller's instantiation(s) and returns the kernel that keeps its columns in dynamic LDS, wave_bytes per wave.
// Registers: 4 waves a workgroup, no LDS.  NT = 0: as many waves (4 at most) as fit in the CU's LDS, all of which it is allowed.
template <class F>
static int trade_tier(grl_handle *h, int n, size_t wave_bytes, int &waves, size_t &lds, F pick) {
    waves = 4; lds = 0;
    if (n <= 2) pick(std::integral_constant<int, 2>{});
    else if (n <= 4) pick(std::integral_constant<int, 4>{});
    else if (n <= 8) pick(std::integral_constant<int, 8>{});
    else if (n <= 16) pick(std::integral_constant<int, 16>{});
    else {
        const void *kern = pick(std::integral_constant<int, 0>{});
        waves = (int)std::min<size_t>(4, TRADE_LDS_BYTES / wave_bytes);
        lds = wave_bytes * waves;
        GRL_HIP(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, TRADE_LDS_BYTES));
    }
    return GRL_OK;
}

// The tape of normals a whole-episode call may bring.  A handle with GRL_F_INJECT_NOISE has no generator to fall back on:
static int trade_tape_check(grl_handle *h, const char *fn, const float *normals_host) {
    if (!normals_host && (h->cfg.flags & GRL_F_INJECT_NOISE))
        return fail(h, GRL_E_INVALID, std::string(fn) + ": a handle with GRL_F_INJECT_NOISE holds the normals of one step; pass a tape");
    return GRL_OK;
}

// cells floats to the device (none: no tape); drained, so the tape is the caller's again when the call returns
static int trade_tape_upload(grl_handle *h, float *tape_dev, const float *normals_host, size_t cells) {
    if (!cells) return GRL_OK;
    GRL_HIP(h, hipMemcpyAsync(tape_dev, normals_host, cells * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));
    return GRL_OK;
}

}  // namespace grl
