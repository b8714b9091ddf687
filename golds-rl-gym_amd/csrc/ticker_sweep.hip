// Scripted rule baseline sweep for the Ticker env: every (env, rule) pair plays a whole episode from the env's current state in
// ONE launch (C ABI: include/goldsrl_tickersweep.h).
//
// Mapping: one lane per pair.  The lanes of a wave are consecutive envs of ONE rule, so the rule's six parameters are wave-uniform
// and the (n_rules, E) outputs store coalesced; the four waves of a workgroup hold four rules of the same 64 envs.  The account
// (cash, q0, q1, assets, log(assets + 1e-4)) and the statistics stay in registers.  No LDS, no barrier, no atomics, no workgroup
// talks to another.  Unlike TradeAR1 the price path costs no pow / exp, only a 16-byte gather from a table that sits in L2, so
// there is nothing for several rules per lane to share: one rule per lane is the only form built.
//
// The row addresses do not depend on the actions: the next step's row and its lookback price are asked for before the current
// step's divide chain.  A step is played only while the window holds the row of the observation that follows it (idx <= 1022),
// which is where the step path raises its window error; so the row asked for ahead (idx + 1 <= 1023) is always inside the window.
//
// The handle's state is read only: nothing here writes the account, idx / start / elapsed / episode / nhist, the outputs, the done
// list, err_flag or the episode records.
#include <math.h>

#include "ticker_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tickersweep.h"

namespace grl {

struct TickerSweepOut {
    PairStats stats;
    double *final_assets;
    int32_t *trades;
    uint8_t *depleted;
    float *trace_r;
    double *trace_a;
    float4 *trace_act;
};

__global__ __launch_bounds__(256) void ticker_sweep_kernel(TickerParams K, const float *__restrict__ rules, int n_rules, int max_steps,
                                                           int trace_env, TickerSweepOut O) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r = blockIdx.y * 4 + wave;                       // wave-uniform
    if (r >= n_rules || env >= K.E) return;
    TickerRule U;
    U.up0 = (double)rules[r * 6 + 0]; U.up1 = (double)rules[r * 6 + 1]; U.dn0 = (double)rules[r * 6 + 2]; U.dn1 = (double)rules[r * 6 + 3];
    U.band = (double)rules[r * 6 + 4]; U.lookback = (int)rules[r * 6 + 5];

    int idx = max(0, min(K.idx[env], TICKER_WINDOW - 1));      // as ticker_step_env: keep the rows inside the table
    const int st = max(0, min(K.start[env], K.rows - TICKER_WINDOW));
    const double *win = K.table + (size_t)st * 4;
    const int el0 = K.elapsed[env];
    const double2 qq = reinterpret_cast<const double2 *>(K.q)[env];
    double cash = K.cash[env], q0 = qq.x, q1 = qq.y, assets = K.assets[env];
    double la = log(assets + 1e-4);
    RewardStats rs;
    int length = 0, trades = 0;
    bool finished = false, depleted = false;
    const bool trace = env == trace_env;
    const size_t tr0 = (size_t)r * max_steps;

    double2 pp = *reinterpret_cast<const double2 *>(win + (size_t)idx * 4);
    double back = win[(size_t)max(idx - U.lookback, 0) * 4];
    for (int t = 0; t < max_steps; ++t) {
        if (idx >= TICKER_WINDOW - 1) break;                   // no row for the observation after this step: the window is played out
        const double2 pn = *reinterpret_cast<const double2 *>(win + (size_t)(idx + 1) * 4);
        const double bn = win[(size_t)max(idx + 1 - U.lookback, 0) * 4];
        const float4 act = ticker_rule_action(U, cash, q0, q1, pp.x, pp.y, back);
        const float rew = ticker_account_step(act, pp.x, pp.y, cash, q0, q1, assets, la);
        rs.add(rew);
        length = t + 1;
        trades += (act.x != 0.f || act.y != 0.f) ? 1 : 0;
        if (trace) {
            O.trace_r[tr0 + t] = rew;
            O.trace_a[tr0 + t] = assets;
            O.trace_act[tr0 + t] = act;
        }
        depleted = assets < TICKER_MIN_CASH;
        finished = depleted || (K.max_steps > 0 && el0 + t + 1 >= K.max_steps);
        if (finished) break;
        idx += 1;
        pp = pn;
        back = bn;
    }
    const size_t o = (size_t)r * K.E + env;
    O.stats.store(o, rs, length, finished);
    O.final_assets[o] = assets; O.trades[o] = trades;
    O.depleted[o] = depleted ? 1 : 0;
}

// the first thing wrong with rule i, or nullptr
static const char *ticker_rule_fault(const float *u, const char **field) {
    static const char *names[6] = {"up0", "up1", "dn0", "dn1", "band", "lookback"};
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(u[k])) { *field = names[k]; return "is not finite"; }
    for (int k = 0; k < 4; ++k)
        if (u[k] < 0.f || u[k] > 1.f) { *field = names[k]; return "is a weight outside [0, 1]"; }
    if ((double)u[0] + (double)u[1] > 1.0) { *field = "up0 + up1"; return "is above 1"; }
    if ((double)u[2] + (double)u[3] > 1.0) { *field = "dn0 + dn1"; return "is above 1"; }
    if (u[4] < 0.f) { *field = names[4]; return "is negative"; }
    if (u[5] < 0.f || u[5] > (float)(TICKER_WINDOW - 1) || u[5] != floorf(u[5])) { *field = names[5]; return "is not an integer in 0..1023"; }
    return nullptr;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_ticker_sweep(grl_handle *h, const float *rules_host, int32_t n_rules, int32_t max_steps, int32_t trace_env) {
    const char *fn = "grl_ticker_sweep";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TICKER, "Ticker", rules_host))) return rc;
    if (!h->tk.table) return fail(h, GRL_E_INVALID, "grl_ticker_sweep: the handle has no price table yet (grl_ticker_set_table first)");
    if ((rc = episode_check_count(h, fn, "n_rules", n_rules, 4096)) || (rc = episode_check_steps(h, fn, max_steps)) ||
        (rc = episode_check_trace_env(h, fn, trace_env)))
        return rc;
    for (int i = 0; i < n_rules; ++i) {
        const char *field = nullptr, *what = ticker_rule_fault(rules_host + (size_t)i * 6, &field);
        if (what) return fail(h, GRL_E_INVALID, "grl_ticker_sweep: rule " + std::to_string(i) + ": " + field + " " + what);
    }
    if ((rc = episode_check_idle(h, fn))) return rc;
    hipSetDevice(h->cfg.device_id);
    TickerSweepState &w = h->ksw;
    w.n_rules = 0;
    const size_t pairs = (size_t)n_rules * h->E, trace = trace_env >= 0 ? (size_t)n_rules * max_steps : 0;
    if ((rc = episode_reserve(h, w.cap_rules, n_rules, {buf(w.rules, 6)})) ||
        (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.final_assets), buf(w.trades), buf(w.depleted)}, &w.stats)) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_r), buf(w.trace_a), buf(w.trace_act, 4)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.rules, rules_host, (size_t)n_rules * 6 * 4, hipMemcpyHostToDevice, h->stream));
    if (trace) {     // rows are defined up to the pair's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(w.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_a, 0, trace * 8, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_act, 0, trace * 16, h->stream));
    }
    const TickerParams K = ticker_params(h);
    TickerSweepOut O{};
    O.stats = w.stats; O.final_assets = w.final_assets; O.trades = w.trades; O.depleted = w.depleted;
    O.trace_r = w.trace_r; O.trace_a = w.trace_a; O.trace_act = reinterpret_cast<float4 *>(w.trace_act);
    const dim3 grid((h->E + 63) / 64, (n_rules + 3) / 4), block(256);
    rc = episode_launch(h, [&] { hipLaunchKernelGGL(ticker_sweep_kernel, grid, block, 0, h->stream, K, w.rules, n_rules, max_steps, trace_env, O); });
    if (rc) return rc;
    w.n_rules = n_rules; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_ticker_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TickerSweepState &w = h->ksw;
    const size_t pairs = (size_t)w.n_rules * h->E, trace = (size_t)w.n_rules * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last sweep traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"final_assets", w.final_assets, pairs * 8}, {"trades", w.trades, pairs * 4}, {"depleted", w.depleted, pairs},
        {"trace_rewards", w.trace_r, trace * 4, untraced}, {"trace_assets", w.trace_a, trace * 8, untraced},
        {"trace_actions", w.trace_act, trace * 16, untraced}};
    return episode_read(h, "grl_ticker_sweep_read", GRL_ENV_TICKER, "Ticker", w.n_rules != 0, "grl_ticker_sweep", outs, nullptr, which, host, bytes, &w.stats, pairs);
}

}  // extern "C"
