// The ceiling of the Ticker env: every (env, horizon) pair plays a whole episode with H rows of foresight (H = 0: the whole episode)
// from the env's current state in ONE launch (C ABI and the recurrence: include/goldsrl_tickerforesight.h).
//
// Mapping: that of ticker_sweep_kernel.  One lane per pair; the lanes of a wave are consecutive envs of ONE horizon, so H and the
// branch between the two forms are wave-uniform and the (n_horizons, E) outputs store coalesced; the four waves of a workgroup hold
// four horizons of the same 64 envs.  The account and the statistics stay in registers; the step is ticker_account_step.  No LDS, no
// barrier, no atomics.
//
// H > 0: every step runs its backward loop over at most H rows in registers.  The row addresses do not depend on the arithmetic, so
// each iteration asks for the row of the next one (16 bytes, the table sits in L2) before its own two divisions.
// H = 0: the known rows of every step end at the episode's last row, so ONE backward pass gives every step's decision.  It stores
// a decision byte per step in a (max_steps, pairs) buffer -- consecutive lanes, consecutive bytes -- and the forward play reads
// them back, each byte by the lane that wrote it, a step ahead of its use.
//
// The handle's state is read only: nothing here writes the account, idx / start / elapsed / episode / nhist, the outputs, the done
// list, err_flag or the episode records.
#include <math.h>

#include "ticker_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tickerforesight.h"

namespace grl {

struct TickerForesightOut {
    PairStats stats;
    double *final_assets, *bound;
    int32_t *trades;
    uint8_t *depleted;
    float *trace_r;
    double *trace_a;
    float4 *trace_act;
    uint8_t *dec;
};

// one row of the backward recurrence, one IEEE operation per line.  Returns choice0 | choice1 << 2 of the row.
__device__ __forceinline__ int ticker_foresight_row(double p0, double p1, double &A, double &B0, double &B1) {
    const double up = 1.0 + TICKER_SPREAD, dn = 1.0 - TICKER_SPREAD;
    const double a0 = p0 * up;
    const double a1 = p1 * up;
    const double x0 = B0 / a0;
    const double x1 = B1 / a1;
    const double b0 = p0 * dn;
    const double b1 = p1 * dn;
    const double y0 = b0 * A;
    const double y1 = b1 * A;
    double An = A;
    int c0 = 0, c1 = 0;
    if (x0 > An) { An = x0; c0 = 1; }
    if (x1 > An) { An = x1; c0 = 0; c1 = 1; }
    if (y0 > B0) { B0 = y0; c0 = c0 ? c0 : 2; }
    if (y1 > B1) { B1 = y1; c1 = c1 ? c1 : 2; }
    A = An;
    return c0 | (c1 << 2);
}

__global__ __launch_bounds__(256) void ticker_foresight_kernel(TickerParams K, const int32_t *__restrict__ horizons, int n_horizons,
                                                               int max_steps, int trace_env, TickerForesightOut O) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r = blockIdx.y * 4 + wave;                       // wave-uniform
    if (r >= n_horizons || env >= K.E) return;
    const int H = horizons[r];                                 // wave-uniform

    const int idx = max(0, min(K.idx[env], TICKER_WINDOW - 1));    // as ticker_step_env: keep the rows inside the table
    const int st = max(0, min(K.start[env], K.rows - TICKER_WINDOW));
    const double2 *win = reinterpret_cast<const double2 *>(K.table + (size_t)st * 4);      // row j of the window: win[2 * j]
    const int el0 = K.elapsed[env];
    const double2 qq = reinterpret_cast<const double2 *>(K.q)[env];
    double cash = K.cash[env], q0 = qq.x, q1 = qq.y, assets = K.assets[env];
    double la = log(assets + 1e-4);
    // the steps of the pair, depletion aside: rows idx .. idx + n - 1, all at or below 1022
    int n = min(max_steps, TICKER_WINDOW - 1 - idx);
    if (K.max_steps > 0) n = min(n, max(K.max_steps - el0, 1));
    const int last = idx + n - 1;
    const size_t pairs = (size_t)n_horizons * K.E;
    const size_t o = (size_t)r * K.E + env;

    double bound = __builtin_nan("");
    if (H == 0) {                                              // the plan of the whole episode, last row first
        double2 row = win[2 * max(last, idx)];
        double A = 1.0, B0 = row.x, B1 = row.y;
        for (int t = n - 1; t >= 0; --t) {
            const double2 nx = win[2 * (idx + max(t - 1, 0))];
            const int d = ticker_foresight_row(row.x, row.y, A, B0, B1);
            O.dec[(size_t)t * pairs + o] = (uint8_t)d;
            row = nx;
        }
        const double vc = cash * A;
        const double v0 = q0 * B0;
        const double v1 = q1 * B1;
        const double vs = vc + v0;
        const double v = vs + v1;
        bound = log(v + 1e-4) - la;
    }

    RewardStats rs;
    int length = 0, trades = 0;
    bool finished = false, depleted = false;
    const bool trace = env == trace_env;
    const size_t tr0 = (size_t)r * max_steps;

    double2 pp = win[2 * idx];
    int d = (H == 0 && n > 0) ? O.dec[o] : 0;
    for (int t = 0; t < n; ++t) {
        const int i = idx + t;
        const double2 pn = win[2 * (i + 1)];                   // i <= 1022: inside the window
        int dnext = 0;
        if (H == 0) {
            if (t + 1 < n) dnext = O.dec[(size_t)(t + 1) * pairs + o];
        } else {
            const int e = min(i + H, last);
            double2 row = win[2 * e];
            double A = 1.0, B0 = row.x, B1 = row.y;
            for (int j = e; j > i; --j) {
                const double2 nx = win[2 * (j - 1)];
                ticker_foresight_row(row.x, row.y, A, B0, B1);
                row = nx;
            }
            d = ticker_foresight_row(pp.x, pp.y, A, B0, B1);
        }
        const int c0 = d & 3, c1 = d >> 2;
        const float4 act = make_float4((float)c0, (float)c1, c0 ? 1.f : 0.f, c1 ? 1.f : 0.f);
        const float rew = ticker_account_step(act, pp.x, pp.y, cash, q0, q1, assets, la);
        rs.add(rew);
        length = t + 1;
        trades += d != 0 ? 1 : 0;
        if (trace) {
            O.trace_r[tr0 + t] = rew;
            O.trace_a[tr0 + t] = assets;
            O.trace_act[tr0 + t] = act;
        }
        depleted = assets < TICKER_MIN_CASH;
        finished = depleted || (K.max_steps > 0 && el0 + t + 1 >= K.max_steps);
        if (finished) break;
        pp = pn;
        d = dnext;
    }
    O.stats.store(o, rs, length, finished);
    O.final_assets[o] = assets; O.bound[o] = bound; O.trades[o] = trades;
    O.depleted[o] = depleted ? 1 : 0;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_ticker_foresight(grl_handle *h, const int32_t *horizons, int32_t n_horizons, int32_t max_steps, int32_t trace_env) {
    const char *fn = "grl_ticker_foresight";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TICKER, "Ticker", horizons))) return rc;
    if (!h->tk.table) return fail(h, GRL_E_INVALID, "grl_ticker_foresight: the handle has no price table yet (grl_ticker_set_table first)");
    if ((rc = episode_check_count(h, fn, "n_horizons", n_horizons, 64)) || (rc = episode_check_steps(h, fn, max_steps)) ||
        (rc = episode_check_trace_env(h, fn, trace_env)))
        return rc;
    bool whole = false;
    for (int i = 0; i < n_horizons; ++i) {
        if (horizons[i] < 0 || horizons[i] > TICKER_WINDOW - 1)
            return fail(h, GRL_E_INVALID, "grl_ticker_foresight: horizon " + std::to_string(i) + " is not 0 (the whole episode) or in 1..1023");
        whole = whole || horizons[i] == 0;
    }
    if ((rc = episode_check_idle(h, fn))) return rc;
    hipSetDevice(h->cfg.device_id);
    TickerForesightState &w = h->kfs;
    w.n_horizons = 0;
    const size_t pairs = (size_t)n_horizons * h->E, trace = trace_env >= 0 ? (size_t)n_horizons * max_steps : 0;
    const size_t dec = whole ? (size_t)max_steps * pairs : 0;
    if ((rc = episode_reserve(h, w.cap_h, n_horizons, {buf(w.horizons)})) ||
        (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.final_assets), buf(w.bound), buf(w.trades), buf(w.depleted)}, &w.stats)) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_r), buf(w.trace_a), buf(w.trace_act, 4)})) ||
        (rc = episode_reserve(h, w.cap_dec, dec, {buf(w.decisions)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.horizons, horizons, (size_t)n_horizons * 4, hipMemcpyHostToDevice, h->stream));
    if (trace) {     // rows are defined up to the pair's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(w.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_a, 0, trace * 8, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_act, 0, trace * 16, h->stream));
    }
    const TickerParams K = ticker_params(h);
    TickerForesightOut O{};
    O.stats = w.stats; O.final_assets = w.final_assets; O.bound = w.bound; O.trades = w.trades; O.depleted = w.depleted; O.dec = w.decisions;
    O.trace_r = w.trace_r; O.trace_a = w.trace_a; O.trace_act = reinterpret_cast<float4 *>(w.trace_act);
    const dim3 grid((h->E + 63) / 64, (n_horizons + 3) / 4), block(256);
    rc = episode_launch(h, [&] { hipLaunchKernelGGL(ticker_foresight_kernel, grid, block, 0, h->stream, K, w.horizons, n_horizons, max_steps, trace_env, O); });
    if (rc) return rc;
    w.n_horizons = n_horizons; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_ticker_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TickerForesightState &w = h->kfs;
    const size_t pairs = (size_t)w.n_horizons * h->E, trace = (size_t)w.n_horizons * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last call traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"final_assets", w.final_assets, pairs * 8}, {"bound", w.bound, pairs * 8}, {"trades", w.trades, pairs * 4},
        {"depleted", w.depleted, pairs},
        {"trace_rewards", w.trace_r, trace * 4, untraced}, {"trace_assets", w.trace_a, trace * 8, untraced},
        {"trace_actions", w.trace_act, trace * 16, untraced}};
    return episode_read(h, "grl_ticker_foresight_read", GRL_ENV_TICKER, "Ticker", w.n_horizons != 0, "grl_ticker_foresight", outs, nullptr, which, host,
                        bytes, &w.stats, pairs);
}

}  // extern "C"
