// Scripted rule baseline sweep for the Ticker env: every (env, rule) pair plays a whole episode from the env's current state in
// ONE launch (C ABI: include/goldsrl_tickersweep.h).
//
// Mapping: one lane per pair.  The lanes of a wave are consecutive envs of ONE rule, so the rule's six parameters are wave-uniform
// and the (n_rules, E) outputs store coalesced; the four waves of a workgroup hold four rules of the same 64 envs.  The account
// (cash, q0, q1, assets, log(assets + 1e-4)) and the statistics stay in registers.  No LDS, no barrier, no atomics, no workgroup
// talks to another.  Unlike TradeAR1 the price path costs no pow / exp, only a 16-byte gather from a table that sits in L2, so
// there is nothing for several rules per lane to share: one rule per lane is the only form built.
//
// The step loop is ticker_sweep_play of ticker_sweep_dev.h, which the rule search (ticker_search.hip) instantiates as well; what this
// kernel keeps of a pair is TickerSweepSink below.
//
// The handle's state is read only: nothing here writes the account, idx / start / elapsed / episode / nhist, the outputs, the done
// list, err_flag or the episode records.
#include <math.h>

#include "ticker_sweep_dev.h"
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

// what the sweep keeps of a pair: the statistics and the trades in registers, the traced env's steps, the final account
struct TickerSweepSink {
    const TickerSweepOut &O;
    const size_t o, tr0;                                       // the pair's slot; its first trace row
    const bool trace;
    RewardStats rs;
    int trades = 0;
    __device__ __forceinline__ void step(int t, const float4 act, float rew, double assets) {
        rs.add(rew);
        trades += (act.x != 0.f || act.y != 0.f) ? 1 : 0;
        if (trace) {
            O.trace_r[tr0 + t] = rew;
            O.trace_a[tr0 + t] = assets;
            O.trace_act[tr0 + t] = act;
        }
    }
    __device__ __forceinline__ void finish(int length, bool finished, bool depleted, double assets) {
        O.stats.store(o, rs, length, finished);
        O.final_assets[o] = assets; O.trades[o] = trades;
        O.depleted[o] = depleted ? 1 : 0;
    }
};

__global__ __launch_bounds__(256) void ticker_sweep_kernel(TickerParams K, const float *__restrict__ rules, int n_rules, int max_steps,
                                                           int trace_env, TickerSweepOut O) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r = blockIdx.y * 4 + wave;                       // wave-uniform
    if (r >= n_rules || env >= K.E) return;
    const TickerRule U = ticker_rule_load(rules, r);
    TickerSweepSink S{O, (size_t)r * K.E + env, (size_t)r * max_steps, env == trace_env};
    ticker_sweep_play(K, U, env, max_steps, S);
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
