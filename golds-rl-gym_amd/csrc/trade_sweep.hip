// Scripted trading-rule baseline sweep for TradeAR1: every (env, rule) pair plays a whole episode from the env's current state in
// ONE launch (C ABI: include/goldsrl_tradesweep.h).
//
// Mapping (that of solow_sweep.hip): one lane per env, RPL rules per lane.  The price path does not depend on the actions, so the
// lane draws the normals and runs pow / exp once per asset and step and carries RPL accounts (cash, assets, q[n]) over it; the
// rule's action, the trade and the two logs of the reward run per rule.  Lanes of a wave are consecutive envs; the waves of a
// workgroup hold rule groups of the SAME 64 envs.  No workgroup talks to another, there is no barrier.
//
// Where p and q live: up to 16 assets in registers, in compile-time tiers NT = 2 / 4 / 8 / 16 whose loops are fully unrolled under
// a uniform `a < n` guard (no runtime register index, no arithmetic on the unused slots).  From 17 to 64 assets (NT = 0) they are
// LDS columns [asset][lane] of the lane's wave, (1 + RPL) * n * 512 bytes per wave; the workgroup has as many waves (4 at most)
// as fit in the CU's 160 KB, one at 64 assets and RPL 4.  Either way the handle's global memory is read once at entry.
//
// The handle's state is read only: nothing here writes cash, assets, q, p, nstep, elapsed, the outputs, the done list or the
// episode records.
#include <math.h>
#include <stdlib.h>

#include "trade_sweep_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tradesweep.h"

namespace grl {

struct TradeSweepOut {
    PairStats stats;
    double *final_assets;
    uint8_t *depleted;
    float *trace_r;
    double *trace_a;
};

// what the sweep keeps of a lane's RPL pairs: the statistics of the step rewards, the trace of one env, the final account
template <int RPL>
struct TradeSweepSink {
    RewardStats rs[RPL];
    const TradeSweepOut &O;
    size_t E;
    int env, r0, n_rules, max_steps;
    bool trace;
    __device__ __forceinline__ void step(int j, int t, float rew, double assets) {
        rs[j].add(rew);
        if (trace && r0 + j < n_rules) {
            O.trace_r[(size_t)(r0 + j) * max_steps + t] = rew;
            O.trace_a[(size_t)(r0 + j) * max_steps + t] = assets;
        }
    }
    __device__ __forceinline__ void finish(int j, int length, bool finished, bool depleted, double assets) {
        if (r0 + j < n_rules) {
            const size_t o = (size_t)(r0 + j) * E + env;
            O.stats.store(o, rs[j], length, finished);
            O.final_assets[o] = assets; O.depleted[o] = depleted ? 1 : 0;
        }
    }
};

// the step loop is trade_sweep_play's (trade_sweep_dev.h), which the search's evaluation instantiates too
template <int RPL, int NT>
__global__ __launch_bounds__(256) void trade_sweep_kernel(TradeParams R, const float *__restrict__ gains, const float *__restrict__ biases,
                                                          int n_rules, const float *__restrict__ tape, int max_steps, int trace_env,
                                                          TradeSweepOut O) {
    extern __shared__ double tsw_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r0 = (blockIdx.y * waves + wave) * RPL;          // wave-uniform
    if (r0 >= n_rules || env >= R.E) return;
    TradeRule2 U[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        const int r = r0 + j < n_rules ? r0 + j : n_rules - 1;             // a ragged tail replays the last rule and stores nothing
        U[j].gain = (double)gains[r]; U[j].bias = (double)biases[r];
    }
    TradeSweepSink<RPL> S{{}, O, (size_t)R.E, env, r0, n_rules, max_steps, env == trace_env};
    trade_sweep_play<RPL, NT>(R, U, tape, env, tsw_lds + (size_t)wave * (1 + RPL) * R.n * 64 + lane, max_steps, S);
}

// rules per lane: 2 is the measured best of 1 / 2 / 4 at 9 rules x 1 024 steps x 8 192 envs (4.40 / 3.32 / 5.03 ms at 2 assets,
// 28.2 / 18.7 / 25.6 ms at 16; profiles/trade_sweep_times.json): one rule per lane pays the float64 pow / exp of the price path
// once per rule, four leave 3 of the 9 rules' slots idle in the ragged group and run at 256 registers.  At 4 096 envs and below
// the pairs do not fill the SIMDs and 1 is faster (2.60 / 3.30 / 5.03 ms at 2 assets).  GRL_TRADE_SWEEP_RPL picks another for that
// measurement and for the tests.  Every value gives the same bits.
static int trade_sweep_rpl() {
    const char *v = getenv("GRL_TRADE_SWEEP_RPL");
    if (v && (v[0] == '1' || v[0] == '2' || v[0] == '4') && v[1] == 0) return v[0] - '0';
    return 2;
}

template <int RPL>
static int trade_sweep_launch(grl_handle *h, const TradeParams &R, int n_rules, const float *tape, int max_steps, int trace_env,
                              const TradeSweepOut &O) {
    const TradeSweepState &w = h->tsw;
    const int n = R.n, groups = (n_rules + RPL - 1) / RPL;
    int waves; size_t lds;
    void (*kern)(TradeParams, const float *, const float *, int, const float *, int, int, TradeSweepOut);
    const size_t per_wave = (size_t)(1 + RPL) * n * 64 * sizeof(double);           // at most 5 * 64 * 512 = 160 KB
    const int rc = trade_tier(h, n, per_wave, waves, lds, [&](auto nt) { return (const void *)(kern = trade_sweep_kernel<RPL, decltype(nt)::value>); });
    if (rc) return rc;
    const dim3 grid((h->E + 63) / 64, (groups + waves - 1) / waves), block(64 * waves);
    return episode_launch(h, [&] { hipLaunchKernelGGL(kern, grid, block, lds, h->stream, R, w.gains, w.biases, n_rules, tape, max_steps, trace_env, O); });
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_trade_sweep(grl_handle *h, const float *gains_host, const float *biases_host, int32_t n_rules, const float *normals_host,
                    int32_t max_steps, int32_t trace_env) {
    const char *fn = "grl_trade_sweep";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TRADE, "TradeAR1", gains_host && biases_host)) || (rc = episode_check_count(h, fn, "n_rules", n_rules, 4096)) ||
        (rc = episode_check_steps(h, fn, max_steps)) || (rc = episode_check_trace_env(h, fn, trace_env)))
        return rc;
    for (int i = 0; i < n_rules; ++i)
        if (!std::isfinite(gains_host[i]) || !std::isfinite(biases_host[i]))
            return fail(h, GRL_E_INVALID, "grl_trade_sweep: rule " + std::to_string(i) + " has a non-finite gain or bias");
    if ((rc = trade_tape_check(h, fn, normals_host)) || (rc = episode_check_idle(h, fn))) return rc;
    hipSetDevice(h->cfg.device_id);
    TradeSweepState &w = h->tsw;
    w.n_rules = 0;
    const size_t pairs = (size_t)n_rules * h->E, trace = trace_env >= 0 ? (size_t)n_rules * max_steps : 0;
    const size_t tape = normals_host ? (size_t)max_steps * h->cfg.n_assets * h->E : 0;
    if ((rc = episode_reserve(h, w.cap_rules, n_rules, {buf(w.gains), buf(w.biases)})) ||
        (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.final_assets), buf(w.depleted)}, &w.stats)) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_r), buf(w.trace_a)})) || (rc = episode_reserve(h, w.cap_tape, tape, {buf(w.tape)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.gains, gains_host, (size_t)n_rules * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.biases, biases_host, (size_t)n_rules * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = trade_tape_upload(h, w.tape, normals_host, tape))) return rc;
    if (trace) {     // rows are defined up to the pair's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(w.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_a, 0, trace * 8, h->stream));
    }
    const TradeParams R = trade_params(h);
    TradeSweepOut O{};
    O.stats = w.stats; O.final_assets = w.final_assets; O.depleted = w.depleted; O.trace_r = w.trace_r; O.trace_a = w.trace_a;
    const float *tp = tape ? w.tape : nullptr;
    const int rpl = trade_sweep_rpl();
    if (rpl == 1) rc = trade_sweep_launch<1>(h, R, n_rules, tp, max_steps, trace_env, O);
    else if (rpl == 2) rc = trade_sweep_launch<2>(h, R, n_rules, tp, max_steps, trace_env, O);
    else rc = trade_sweep_launch<4>(h, R, n_rules, tp, max_steps, trace_env, O);
    if (rc) return rc;
    w.n_rules = n_rules; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_trade_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TradeSweepState &w = h->tsw;
    const size_t pairs = (size_t)w.n_rules * h->E, trace = (size_t)w.n_rules * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last sweep traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"final_assets", w.final_assets, pairs * 8}, {"depleted", w.depleted, pairs},
        {"trace_rewards", w.trace_r, trace * 4, untraced}, {"trace_assets", w.trace_a, trace * 8, untraced}};
    return episode_read(h, "grl_trade_sweep_read", GRL_ENV_TRADE, "TradeAR1", w.n_rules != 0, "grl_trade_sweep", outs, nullptr, which, host, bytes, &w.stats, pairs);
}

}  // extern "C"
