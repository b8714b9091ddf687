// The step loop of the TradeAR1 whole-episode rule kernels, once: one lane plays RPL rules over ONE price path of its env, from the
// env's current state until max_steps, the TimeLimit or depletion.  trade_sweep.hip instantiates it over the (gain, bias) rule and
// the sweep's statistics, trace and final account, trade_search.hip over the four-number rule and one running total per pair; what
// a pair keeps is the sink's business, the steps are the same statements (trade_asset_trade, trade_account_settle,
// trade_prices_step of flat_env_dev.h) in the same order.
//
// Where p and q live is the caller's tier NT (flat_env_dev.h): registers for NT = 2 / 4 / 8 / 16, or, NT = 0, LDS columns
// [asset][lane] of the lane's wave -- `col` is the lane's slot of its wave's (1 + RPL) * n * 64 doubles, p at col[a * 64], q of rule j
// at col[((1 + j) * n + a) * 64] (unread with NT > 0).  No workgroup talks to another, there is no barrier.
//
// The handle's state is read only: nothing here writes cash, assets, q, p, nstep, elapsed, the outputs, the done list or the
// episode records.
#pragma once
#include <math.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"

namespace grl {

// the sweep's rule (include/goldsrl_tradesweep.h), widened as it is played
struct TradeRule2 {
    double gain, bias;
    __device__ __forceinline__ float action(double p) const { return trade_rule_action(gain, bias, p); }
};

// the search's rule (include/goldsrl_tradesearch.h), row r of a (n_rules, 4) float32 table
struct TradeRule4 {
    double gain_buy, gain_sell, bias, ref;
    __device__ __forceinline__ float action(double p) const { return trade_rule4_action(gain_buy, gain_sell, bias, ref, p); }
};

__device__ __forceinline__ TradeRule4 trade_rule4_load(const float *__restrict__ rules, int r) {
    const float4 f = reinterpret_cast<const float4 *>(rules)[r];
    return TradeRule4{(double)f.x, (double)f.y, (double)f.z, (double)f.w};
}

// Rule: action(p), the float32 action for an asset at price p.  Sink: step(j, t, rew, assets) after every step rule slot j plays,
// in step order; finish(j, length, finished, depleted, assets) once per slot, in slot order, after the loop.  A caller whose last
// group is ragged fills the spare slots with a copy of a real rule and has its sink drop them.
template <int RPL, int NT, class Rule, class Sink>
__device__ __forceinline__ void trade_sweep_play(const TradeParams &R, const Rule (&U)[RPL], const float *__restrict__ tape, int env, double *col,
                                                 int max_steps, Sink &S) {
    constexpr bool REG = NT > 0;
    constexpr int NR = REG ? NT : 1;
    const size_t E = R.E;
    const int n = R.n, pairs = (n + 1) / 2;

    double pr[NR], qr[RPL][NR];
    auto P = [&](int a) -> double & { if constexpr (REG) return pr[a]; else return col[(size_t)a * 64]; };
    auto Q = [&](int j, int a) -> double & { if constexpr (REG) return qr[j][a]; else return col[((size_t)(1 + j) * n + a) * 64]; };

    double cash[RPL], assets[RPL];
    int length[RPL];
    bool live[RPL], finished[RPL], depleted[RPL];
    const double cash0 = R.cash[env], assets0 = R.assets[env];
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        cash[j] = cash0; assets[j] = assets0;
        length[j] = 0; live[j] = true; finished[j] = false; depleted[j] = false;
    }
    trade_for<NT>(n, [&](int a) {
        P(a) = R.p[a * E + env];
        const double q0 = R.q[a * E + env];
#pragma unroll
        for (int j = 0; j < RPL; ++j) Q(j, a) = q0;
    });
    const uint32_t st0 = R.nstep[env];
    const int el0 = R.elapsed[env];

    for (int t = 0; t < max_steps; ++t) {
        const bool last = R.max_steps > 0 && el0 + t + 1 >= R.max_steps;   // the TimeLimit ends every rule of the env at this step
        bool any = false;
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            if (!live[j]) continue;
            double cost = 0.0, value = 0.0;
            const double c = cash[j];
            trade_for<NT>(n, [&](int a) {
                const double p = P(a);
                trade_asset_trade(U[j].action(p), n, c, p, Q(j, a), cost, value);
            });
            bool dep;
            const float rew = trade_account_settle(cash[j], assets[j], cost, value, dep);
            length[j] = t + 1;
            S.step(j, t, rew, assets[j]);
            depleted[j] = dep;
            finished[j] = dep || last;
            live[j] = !finished[j];
            any |= live[j];
        }
        if (!any || t + 1 == max_steps) break;
        // _price_transition of every asset, once for all rules of the lane
        trade_prices_step<NT>(R, tape, env, st0, t, pairs, [&](int a) { return P(a); }, [&](int a, double p) { P(a) = p; });
    }
#pragma unroll
    for (int j = 0; j < RPL; ++j) S.finish(j, length[j], finished[j], depleted[j], assets[j]);
}

}  // namespace grl
