// The step loop of the Ticker whole-episode rule kernels, once: one (env, rule) pair plays from the env's current state until
// max_steps, the TimeLimit, depletion or the end of the window.  ticker_sweep.hip instantiates it over the sweep's statistics, trace
// and final account, ticker_search.hip over one running total; what a pair keeps is the sink's business, the steps are the same
// statements (ticker_rule_action, ticker_account_step of ticker_dev.h) in the same order.  Also here: the host's check of a rule row,
// which both entry points apply.
//
// The row addresses do not depend on the actions: the next step's row and its lookback price are asked for before the current
// step's divide chain.  A step is played only while the window holds the row of the observation that follows it (idx <= 1022),
// which is where the step path raises its window error; so the row asked for ahead (idx + 1 <= 1023) is always inside the window.
//
// The handle's state is read only: nothing here writes the account, idx / start / elapsed / episode / nhist, the outputs, the done
// list, err_flag or the episode records.
#pragma once
#include <math.h>

#include "ticker_dev.h"

namespace grl {

// row r of a (n_rules, 6) float32 table, widened as the rule is played
__device__ __forceinline__ TickerRule ticker_rule_load(const float *__restrict__ rules, int r) {
    TickerRule U;
    U.up0 = (double)rules[r * 6 + 0]; U.up1 = (double)rules[r * 6 + 1]; U.dn0 = (double)rules[r * 6 + 2]; U.dn1 = (double)rules[r * 6 + 3];
    U.band = (double)rules[r * 6 + 4]; U.lookback = (int)rules[r * 6 + 5];
    return U;
}

// Sink: step(t, act, rew, assets) after every step played, in step order; finish(length, finished, depleted, assets) once.
template <typename Sink>
__device__ __forceinline__ void ticker_sweep_play(const TickerParams &K, const TickerRule &U, int env, int max_steps, Sink &S) {
    int idx = max(0, min(K.idx[env], TICKER_WINDOW - 1));      // as ticker_step_env: keep the rows inside the table
    const int st = max(0, min(K.start[env], K.rows - TICKER_WINDOW));
    const double *win = K.table + (size_t)st * 4;
    const int el0 = K.elapsed[env];
    const double2 qq = reinterpret_cast<const double2 *>(K.q)[env];
    double cash = K.cash[env], q0 = qq.x, q1 = qq.y, assets = K.assets[env];
    double la = log(assets + 1e-4);
    int length = 0;
    bool finished = false, depleted = false;

    double2 pp = *reinterpret_cast<const double2 *>(win + (size_t)idx * 4);
    double back = win[(size_t)max(idx - U.lookback, 0) * 4];
    for (int t = 0; t < max_steps; ++t) {
        if (idx >= TICKER_WINDOW - 1) break;                   // no row for the observation after this step: the window is played out
        const double2 pn = *reinterpret_cast<const double2 *>(win + (size_t)(idx + 1) * 4);
        const double bn = win[(size_t)max(idx + 1 - U.lookback, 0) * 4];
        const float4 act = ticker_rule_action(U, cash, q0, q1, pp.x, pp.y, back);
        const float rew = ticker_account_step(act, pp.x, pp.y, cash, q0, q1, assets, la);
        length = t + 1;
        S.step(t, act, rew, assets);
        depleted = assets < TICKER_MIN_CASH;
        finished = depleted || (K.max_steps > 0 && el0 + t + 1 >= K.max_steps);
        if (finished) break;
        idx += 1;
        pp = pn;
        back = bn;
    }
    S.finish(length, finished, depleted, assets);
}

// the first thing wrong with the rule row u, or nullptr
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
