// TickerEnv as device functions: the per-env step (with the worker's auto-reset and the processed observation), the reset and the
// observation write, shared by the env kernels of ticker.hip and by the kernels that step a Ticker env from inside another launch
// (the gated trader's one-launch evaluation, net_gated_eval.inc).  The arithmetic is the reference's, in its operation order
// (fed_gym/envs/fed_env.py:110-156); every translation unit that includes this header is built with -ffp-contract=off, which the
// float64 account needs to stay bit-exact against numpy.
#pragma once
#include "common.h"
#include "rng.h"

namespace grl {

constexpr int TICKER_WINDOW = 1024;       // fed_env.py:147  self.data.sample(1024)
constexpr double TICKER_SPREAD = 0.006;   // fed_env.py:105
constexpr double TICKER_MIN_CASH = 1.0;   // fed_env.py:96
constexpr double TICKER_START_BALANCE = 10.0;

struct TickerParams {
    double *cash, *assets, *q;            // q (E,2)
    int32_t *idx, *start, *start0, *nhist;
    const double *table;
    int rows;
    int32_t *elapsed, *episode;
    const float *actions;                 // (E,4): choice0, choice1 (0 hold, 1 buy, 2 sell), fraction0, fraction1
    float *reward;
    double *reward64;
    uint8_t *done;
    float *obs_raw, *obs;                 // (E,7)
    int32_t *done_list, *done_count, *err_flag;
    const int32_t *reset_list, *reset_count;
    int E, rnn, max_steps;
    uint32_t flags, env_off;
    uint64_t seed;
};

struct TickerStepOut {
    float reward;
    bool done;
};

static inline TickerParams ticker_params(grl_handle *h) {
    TickerParams K{};
    K.cash = h->tk.cash; K.assets = h->tk.assets; K.q = h->tk.q; K.idx = h->tk.idx; K.start = h->tk.start; K.start0 = h->tk.start0;
    K.nhist = h->tk.nhist; K.table = h->tk.table; K.rows = h->tk.rows; K.elapsed = h->elapsed; K.episode = h->episode;
    K.reward = h->reward; K.reward64 = h->tk.reward64; K.done = h->done; K.obs_raw = h->tk.obs_raw; K.obs = h->tk.obs;
    K.done_list = h->done_list; K.done_count = h->done_count; K.err_flag = h->err_flag; K.E = h->E; K.rnn = h->cfg.rnn_length;
    K.max_steps = h->cfg.max_episode_steps; K.flags = h->cfg.flags; K.env_off = (uint32_t)h->cfg.env_id_offset; K.seed = h->cfg.seed;
    return K;
}

// [cash, q0, q1, p0, p1, v0, v1] and TickerTraderStateProcessor.process_state of it
__device__ __forceinline__ void ticker_write_obs(const TickerParams &K, int env, double cash, double q0, double q1, const double *row) {
    float *oraw = K.obs_raw + (size_t)env * 7, *o = K.obs + (size_t)env * 7;
    oraw[0] = (float)cash; oraw[1] = (float)q0; oraw[2] = (float)q1;
    oraw[3] = (float)row[0]; oraw[4] = (float)row[1]; oraw[5] = (float)row[2]; oraw[6] = (float)row[3];
    o[0] = (float)log(cash + 1e-4); o[1] = (float)log(q0 + 1.0); o[2] = (float)log(q1 + 1.0);
    o[3] = (float)log(row[0]); o[4] = (float)log(row[1]); o[5] = (float)row[2]; o[6] = (float)row[3];
}

// TickerEnv._reset (fed_env.py:144-156).  The window start is random.randint(0, T - 1024) in the reference
// (sampler.py:38): here a Philox draw keyed by (seed, global env id, episode), or the stored start0 under
// GRL_F_RESET_FROM_SNAPSHOT.
__device__ __forceinline__ int ticker_reset_env(const TickerParams &K, int env) {
    int st;
    if (K.flags & GRL_F_RESET_FROM_SNAPSHOT) {
        st = K.start0[env];
    } else {
        uint32_t ep = (K.flags & GRL_F_RESEED_EACH_RESET) ? 0u : (uint32_t)K.episode[env];
        double u0, u1;
        u01_pair(rng_block(K.seed, (uint32_t)env + K.env_off, ep, RS_TICKER_START, 0u), u0, u1);
        st = (int)(u0 * (double)(K.rows - TICKER_WINDOW + 1));
    }
    st = max(0, min(st, K.rows - TICKER_WINDOW));
    K.start[env] = st;
    K.idx[env] = 0;
    K.cash[env] = TICKER_START_BALANCE;
    K.assets[env] = TICKER_START_BALANCE;
    reinterpret_cast<double2 *>(K.q)[env] = make_double2(0.0, 0.0);
    K.elapsed[env] = 0;
    K.episode[env] = K.episode[env] + 1;
    return st;
}

// One step of env `env` with act = (choice0, choice1, fraction0, fraction1): TickerEnv._step (fed_env.py:110-142) in the same
// operation order, the TimeLimit, the auto-reset of a finished env and the observation write.  The caller guarantees env < K.E.
__device__ __forceinline__ TickerStepOut ticker_step_env(const TickerParams &K, int env, const float4 act) {
    const int d0 = (int)act.x, d1 = (int)act.y;
    double c0 = (double)act.z, c1 = (double)act.w;
    if (!(act.x == 0.f || act.x == 1.f || act.x == 2.f) || !(act.y == 0.f || act.y == 1.f || act.y == 2.f)) atomicAdd(K.err_flag, 1);
    int idx = max(0, min(K.idx[env], TICKER_WINDOW - 1));                    // host-settable fields: keep the row inside the table
    const int st = max(0, min(K.start[env], K.rows - TICKER_WINDOW));
    const double *row = K.table + (size_t)(st + idx) * 4;
    const double p0 = row[0], p1 = row[1];
    const double2 qq = reinterpret_cast<const double2 *>(K.q)[env];
    double cash = K.cash[env], q0 = qq.x, q1 = qq.y;
    const bool b0 = d0 == 1, b1 = d1 == 1, s0 = d0 == 2, s1 = d1 == 2;
    const double bsum = (b0 && b1) ? c0 + c1 : (b0 ? c0 : (b1 ? c1 : 0.0));
    const double denom = fmax(bsum, 1.0);
    if (b0) c0 = c0 / denom;
    if (b1) c1 = c1 / denom;
    const double up = 1.0 + TICKER_SPREAD, dn = 1.0 - TICKER_SPREAD;
    const double a0 = b0 ? c0 * cash / (p0 * up) : (s0 ? -c0 * q0 : 0.0);
    const double a1 = b1 ? c1 * cash / (p1 * up) : (s1 ? -c1 * q1 : 0.0);
    q0 = q0 + a0;
    q1 = q1 + a1;
    const double cb0 = a0 * p0 * up, cb1 = a1 * p1 * up;
    const double cs0 = a0 * (p0 * dn), cs1 = a1 * (p1 * dn);
    const double sb = (b0 && b1) ? cb0 + cb1 : (b0 ? cb0 : (b1 ? cb1 : 0.0));
    const double ss = (s0 && s1) ? cs0 + cs1 : (s0 ? cs0 : (s1 ? cs1 : 0.0));
    cash = cash + (-sb - ss);
    const double old_assets = K.assets[env];
    const double assets = cash + (q0 * p0 + q1 * p1);
    const bool own_done = assets < TICKER_MIN_CASH;
    const double r = log(assets + 1e-4) - log(old_assets + 1e-4);
    K.reward64[env] = r;
    K.reward[env] = (float)r;
    idx += 1;
    int el = K.elapsed[env] + 1;
    const bool done = own_done || (K.max_steps > 0 && el >= K.max_steps);
    if (!done && idx >= TICKER_WINDOW) {       // reference: IndexError on price_vol_data[1024] (no TimeLimit registered)
        atomicAdd(K.err_flag, 1 << 16);
        idx = TICKER_WINDOW - 1;
    }
    K.done[env] = done ? 1 : 0;
    if (done) {   // auto-reset (emulator_runner.py:50-52): the terminal reward stays, the observation is the reset one
        const int nst = ticker_reset_env(K, env);
        K.nhist[env] = 1;
        ticker_write_obs(K, env, TICKER_START_BALANCE, 0.0, 0.0, K.table + (size_t)nst * 4);
    } else {
        K.cash[env] = cash;
        K.assets[env] = assets;
        reinterpret_cast<double2 *>(K.q)[env] = make_double2(q0, q1);
        K.idx[env] = idx;
        K.elapsed[env] = el;
        int nh = K.nhist[env] + 1;
        K.nhist[env] = nh > K.rnn + 1 ? K.rnn + 1 : nh;
        ticker_write_obs(K, env, cash, q0, q1, K.table + (size_t)(st + idx) * 4);
    }
    TickerStepOut out;
    out.reward = (float)r;
    out.done = done;
    return out;
}

// ---- the account on values, for kernels that keep it in registers (ticker_sweep.hip).  ticker_step_env above is the form on the
// handle's arrays; the two are held together bit for bit by tests/test_gpu_ticker_sweep.py.

// a scripted rule (include/goldsrl_tickersweep.h): banded target weights with an optional trend switch, float64
struct TickerRule {
    double up0, up1, dn0, dn1, band;
    int lookback;
};

// one asset of the rule: value v of the position, target weight t.  One IEEE operation per line.
__device__ __forceinline__ void ticker_rule_asset(double v, double t, double band, double total, double cash, float &choice, float &fraction) {
    const double s = v / total;
    const double lo = t - band;
    const double hi = t + band;
    double f = 0.0;
    choice = 0.f;
    if (s < lo) {
        choice = 1.f;
        const double d = t - s;
        const double w = d * total;
        const double c = fmax(cash, 1e-12);
        f = w / c;
        f = fmin(f, 1.0);
    } else if (s > hi) {
        choice = 2.f;
        const double d = s - t;
        f = d / s;
        f = fmin(f, 1.0);
    }
    fraction = (float)f;
}

// the rule's action on what the observation shows (cash, q, the prices the trade executes at) and the price `back`, lookback rows
// before: (choice0, choice1, fraction0, fraction1)
__device__ __forceinline__ float4 ticker_rule_action(const TickerRule &U, double cash, double q0, double q1, double p0, double p1, double back) {
    const bool up = U.lookback == 0 || p0 >= back;
    const double t0 = up ? U.up0 : U.dn0, t1 = up ? U.up1 : U.dn1;
    const double v0 = q0 * p0;
    const double v1 = q1 * p1;
    const double hold = v0 + v1;
    const double total = cash + hold;
    float4 act;
    ticker_rule_asset(v0, t0, U.band, total, cash, act.x, act.z);
    ticker_rule_asset(v1, t1, U.band, total, cash, act.y, act.w);
    return act;
}

// the trade and the equity of ticker_step_env (fed_env.py:110-130) for valid choices, in its operation order.  log_assets is
// log(assets + 1e-4) of the account coming in, and of the account going out afterwards: the step's reward is their difference.
__device__ __forceinline__ float ticker_account_step(const float4 act, double p0, double p1, double &cash, double &q0, double &q1,
                                                     double &assets, double &log_assets) {
    const int d0 = (int)act.x, d1 = (int)act.y;
    double c0 = (double)act.z, c1 = (double)act.w;
    const bool b0 = d0 == 1, b1 = d1 == 1, s0 = d0 == 2, s1 = d1 == 2;
    const double bsum = (b0 && b1) ? c0 + c1 : (b0 ? c0 : (b1 ? c1 : 0.0));
    const double denom = fmax(bsum, 1.0);
    if (b0) c0 = c0 / denom;
    if (b1) c1 = c1 / denom;
    const double up = 1.0 + TICKER_SPREAD, dn = 1.0 - TICKER_SPREAD;
    const double a0 = b0 ? c0 * cash / (p0 * up) : (s0 ? -c0 * q0 : 0.0);
    const double a1 = b1 ? c1 * cash / (p1 * up) : (s1 ? -c1 * q1 : 0.0);
    q0 = q0 + a0;
    q1 = q1 + a1;
    const double cb0 = a0 * p0 * up, cb1 = a1 * p1 * up;
    const double cs0 = a0 * (p0 * dn), cs1 = a1 * (p1 * dn);
    const double sb = (b0 && b1) ? cb0 + cb1 : (b0 ? cb0 : (b1 ? cb1 : 0.0));
    const double ss = (s0 && s1) ? cs0 + cs1 : (s0 ? cs0 : (s1 ? cs1 : 0.0));
    cash = cash + (-sb - ss);
    assets = cash + (q0 * p0 + q1 * p1);
    const double la = log(assets + 1e-4);
    const double r = la - log_assets;
    log_assets = la;
    return (float)r;
}

}  // namespace grl
