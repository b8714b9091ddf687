// The ceiling of the TradeAR1 env: every (env, horizon) pair plays a whole episode with H rows of foresight (H = 0: the whole episode)
// from the env's current state in ONE call of two launches (C ABI and the recurrence: include/goldsrl_tradeforesight.h).
//
// 1. trade_path_kernel: one lane per env, lanes of a wave consecutive envs.  The price path does not depend on the actions, so it is
//    written once, float64 [row][asset][env], with the sweep's own draws (trade_price_normals at st0 + t, or the tape) and the
//    sweep's own trade_price_next.  Rows at or past an env's m are written as zero.  Every horizon -- and the host, through the
//    "prices" output -- then sees the device's own pow / exp bits.
// 2. trade_foresight_kernel: one lane per pair; the lanes of a wave are consecutive envs of ONE horizon, so H and the branch between
//    the two forms are wave-uniform, a path row is n coalesced loads and the (n_horizons, E) outputs store coalesced; the waves of a
//    workgroup hold horizons of the same 64 envs.  No barrier, no atomics.
//
// Where q and B live: in the asset tiers of flat_env_dev.h (trade_for in the kernels, trade_tier on the host).  Up to 16 assets in
// registers, NT = 2 / 4 / 8 / 16, loops fully unrolled under a uniform `a < n` guard, with the row in use and the row asked for next
// in registers too.  From 17 to 64 assets (NT = 0) q and B are LDS columns [asset][lane] of the lane's wave, n * 1 024 bytes per
// wave, and a price is loaded where it is used; the workgroup has as many waves (4 at most) as fit in the CU's 160 KB, two at 64.
//
// H > 0: every step runs its backward loop over at most H + 1 rows.  The row addresses do not depend on the arithmetic, so each
// iteration asks for row j - 1 before row j's divisions.
// H = 0: the known rows of every step end at the episode's last row, so ONE backward pass gives every step's decisions.  It stores a
// decision byte per (step, asset, env) -- consecutive lanes, consecutive bytes -- in the plane of its whole-episode column, and the
// forward play reads them back, each byte by the lane that wrote it.
//
// The handle's state is read only: nothing here writes cash, assets, q, p, nstep, elapsed, the outputs, the done list, err_flag or
// the episode records.
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tradeforesight.h"

namespace grl {

struct TradeForesightOut {
    PairStats stats;
    double *final_assets, *bound;
    int32_t *trades;
    uint8_t *depleted;
    float *trace_r;
    double *trace_a;
    float *trace_act;
    uint8_t *dec;
};

constexpr size_t TFS_MAX_PATH = (size_t)1 << 28;       // max_steps * n_assets * E: 2 GiB of path, 256 MiB per whole-episode plan

// the steps of a pair, depletion aside
__device__ __forceinline__ int trade_foresight_steps(const TradeParams &R, int env, int max_steps) {
    int m = max_steps;
    if (R.max_steps > 0) m = min(m, max(R.max_steps - R.elapsed[env], 1));
    return m;
}

template <int NT>
__global__ __launch_bounds__(256) void trade_path_kernel(TradeParams R, const float *__restrict__ tape, int max_steps, double *path) {
    constexpr bool REG = NT > 0;
    constexpr int NR = REG ? NT : 1;
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= R.E) return;
    const size_t E = R.E;
    const int n = R.n, pairs = (n + 1) / 2;
    const int m = trade_foresight_steps(R, env, max_steps);
    const uint32_t st0 = R.nstep[env];
    double pr[NR];
    double *out = path + env;                                  // row t, asset a: out[(t * n + a) * E]
    // the row before t: in registers, or (17 assets and more) read back by the lane that wrote it
    auto prev = [&](int t, int a) -> double { if constexpr (REG) return pr[a]; else return out[((size_t)(t - 1) * n + a) * E]; };
    auto put = [&](int t, int a, double p) { if constexpr (REG) pr[a] = p; out[((size_t)t * n + a) * E] = p; };
    trade_for<NT>(n, [&](int a) { put(0, a, R.p[a * E + env]); });
    for (int t = 1; t < max_steps; ++t) {
        if (t < m) {
            const uint32_t st = st0 + (uint32_t)(t - 1);   // trade_prices_step written out: as a call it is 0.5 % slower here
            trade_for<(NT + 1) / 2>(pairs, [&](int k) {
                const int a = 2 * k;
                double z0, z1 = 0.0;
                if (tape) {
                    z0 = (double)tape[((size_t)(t - 1) * n + a) * E + env];
                    if (a + 1 < n) z1 = (double)tape[((size_t)(t - 1) * n + a + 1) * E + env];
                } else {
                    trade_price_normals(R.seed, (uint32_t)env + R.env_off, st, pairs, k, z0, z1);   // an odd n discards the last z1
                }
                put(t, a, trade_price_next(prev(t, a), R.std_e, z0));
                if (a + 1 < n) put(t, a + 1, trade_price_next(prev(t, a + 1), R.std_e, z1));   // NT is even: slot a + 1 exists
            });
        } else {
            trade_for<NT>(n, [&](int a) { out[((size_t)t * n + a) * E] = 0.0; });
        }
    }
}

template <int NT>
__global__ __launch_bounds__(256) void trade_foresight_kernel(TradeParams R, const int32_t *__restrict__ horizons, int n_horizons,
                                                              int max_steps, int trace_env, const double *__restrict__ path,
                                                              TradeForesightOut O) {
    extern __shared__ double tfs_lds[];
    constexpr bool REG = NT > 0;
    constexpr int NR = REG ? NT : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r = blockIdx.y * waves + wave;                   // wave-uniform
    if (r >= n_horizons || env >= R.E) return;
    const int H = horizons[r];                                 // wave-uniform
    const size_t E = R.E;
    const int n = R.n;
    const double nd = (double)n;

    double qr[NR], br[NR], pc[NR], pn[NR];
    double *col = tfs_lds + (size_t)wave * 2 * n * 64 + lane;  // LDS form: q at col[a * 64], B at col[(n + a) * 64]
    auto Q = [&](int a) -> double & { if constexpr (REG) return qr[a]; else return col[(size_t)a * 64]; };
    auto B = [&](int a) -> double & { if constexpr (REG) return br[a]; else return col[(size_t)(n + a) * 64]; };
    const double *pth = path + env;                            // row j, asset a: pth[(j * n + a) * E]
    auto load = [&](double (&dst)[NR], int j) {                // registers only: the whole row j
        if constexpr (REG) trade_for<NT>(n, [&](int a) { dst[a] = pth[((size_t)j * n + a) * E]; });
    };
    auto take = [&]() {                                        // the row asked for becomes the row in use
        if constexpr (REG) trade_for<NT>(n, [&](int a) { pc[a] = pn[a]; });
    };
    auto price = [&](int j, int a) -> double { if constexpr (REG) return pc[a]; else return pth[((size_t)j * n + a) * E]; };

    // one row of the backward recurrence, one IEEE operation per line; seen(a, p, c) gets the row's decision for asset a: 0 hold,
    // 1 buy, 2 sell
    auto row = [&](int j, double &A, auto seen) {
        double g = 0.0;
        trade_for<NT>(n, [&](int a) {
            const double p = price(j, a);
            const double b = B(a);
            const double x = b / p;
            const double y = p * A;
            int c = 0;
            if (x > A) {
                const double d = x - A;
                g = g + d;
                c = 1;
            }
            if (y > b) {
                B(a) = y;
                c = 2;
            }
            seen(a, p, c);
        });
        const double s = g / nd;
        A = A + s;
    };
    auto nothing = [](int, double, int) {};

    const int el0 = R.elapsed[env];
    const int m = trade_foresight_steps(R, env, max_steps);
    const int last = m - 1;
    double cash = R.cash[env], assets = R.assets[env];
    trade_for<NT>(n, [&](int a) { Q(a) = R.q[a * E + env]; });
    const size_t o = (size_t)r * E + env;

    double bound = __builtin_nan("");
    const uint8_t *dec = nullptr;
    if (H == 0) {                                              // the plan of the whole episode, last row first
        int z = 0;
        for (int i = 0; i < r; ++i) z += horizons[i] == 0 ? 1 : 0;
        uint8_t *plane = O.dec + (size_t)z * max_steps * n * E + env;     // step t, asset a: plane[(t * n + a) * E]
        dec = plane;
        double A = 1.0;
        load(pc, last);
        trade_for<NT>(n, [&](int a) { B(a) = price(last, a); });
        for (int j = last; j >= 0; --j) {
            load(pn, max(j - 1, 0));
            row(j, A, [&](int a, double, int c) { plane[((size_t)j * n + a) * E] = (uint8_t)c; });
            take();
        }
        double v = cash * A;
        trade_for<NT>(n, [&](int a) {
            const double w = Q(a) * B(a);
            v = v + w;
        });
        bound = log(v + 1e-4) - log(assets + 1e-4);
    }

    RewardStats rs;
    int length = 0, trades = 0;
    bool finished = false, depleted = false;
    const bool trace = env == trace_env;
    const size_t tr0 = (size_t)r * max_steps;

    if (H == 0) load(pn, 0);
    for (int t = 0; t < m; ++t) {
        double cost = 0.0, value = 0.0;
        const double c0 = cash;
        bool traded = false;
        // the trade of asset a at price p under decision c, in asset order
        auto trade = [&](int a, double p, int c) {
            const float act = c == 1 ? 1.0f : (c == 2 ? -1.0f : 0.0f);
            trade_asset_trade(act, n, c0, p, Q(a), cost, value);
            traded |= c != 0;
            if (trace) O.trace_act[(tr0 + t) * n + a] = act;
        };
        if (H == 0) {
            take();
            load(pn, min(t + 1, last));
            trade_for<NT>(n, [&](int a) { trade(a, price(t, a), dec[((size_t)t * n + a) * E]); });
        } else {
            const int e = min(t + H, last);
            double A = 1.0;
            load(pc, e);
            trade_for<NT>(n, [&](int a) { B(a) = price(e, a); });
            for (int j = e; j > t; --j) {
                load(pn, j - 1);
                row(j, A, nothing);
                take();
            }
            row(t, A, trade);
        }
        bool dep;
        const float rew = trade_account_settle(cash, assets, cost, value, dep);
        rs.add(rew);
        length = t + 1;
        trades += traded ? 1 : 0;
        if (trace) {
            O.trace_r[tr0 + t] = rew;
            O.trace_a[tr0 + t] = assets;
        }
        depleted = dep;
        finished = dep || (R.max_steps > 0 && el0 + t + 1 >= R.max_steps);
        if (finished) break;
    }
    O.stats.store(o, rs, length, finished);
    O.final_assets[o] = assets; O.bound[o] = bound; O.trades[o] = trades;
    O.depleted[o] = depleted ? 1 : 0;
}

// GRL_TRADE_FORESIGHT_PATH_ONLY=1: the call stops after the path kernel (tools/trade_foresight_times.py times it that way); the
// outputs of such a call cannot be read
static bool trade_foresight_path_only() {
    const char *v = getenv("GRL_TRADE_FORESIGHT_PATH_ONLY");
    return v && v[0] == '1' && v[1] == 0;
}

static int trade_foresight_launch(grl_handle *h, const TradeParams &R, int n_horizons, const float *tape, int max_steps, int trace_env,
                                  const TradeForesightOut &O, bool path_only) {
    const TradeForesightState &w = h->tfs;
    const int n = R.n;
    int waves; size_t lds;
    void (*pathk)(TradeParams, const float *, int, double *);
    void (*playk)(TradeParams, const int32_t *, int, int, int, const double *, TradeForesightOut);
    const size_t per_wave = (size_t)2 * n * 64 * sizeof(double);                   // at most 2 * 64 * 512 = 64 KB
    int rc = trade_tier(h, n, per_wave, waves, lds, [&](auto nt) {
        pathk = trade_path_kernel<decltype(nt)::value>; return (const void *)(playk = trade_foresight_kernel<decltype(nt)::value>);
    });
    if (rc) return rc;
    rc = episode_launch(h, [&] { hipLaunchKernelGGL(pathk, dim3((h->E + 255) / 256), dim3(256), 0, h->stream, R, tape, max_steps, w.path); });
    if (rc || path_only) return rc;
    const dim3 grid((h->E + 63) / 64, (n_horizons + waves - 1) / waves), block(64 * waves);
    return episode_launch(h, [&] { hipLaunchKernelGGL(playk, grid, block, lds, h->stream, R, w.horizons, n_horizons, max_steps, trace_env, w.path, O); });
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_trade_foresight(grl_handle *h, const int32_t *horizons, int32_t n_horizons, const float *normals_host, int32_t max_steps,
                        int32_t trace_env) {
    const char *fn = "grl_trade_foresight";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TRADE, "TradeAR1", horizons)) || (rc = episode_check_count(h, fn, "n_horizons", n_horizons, 64)) ||
        (rc = episode_check_steps(h, fn, max_steps)) || (rc = episode_check_trace_env(h, fn, trace_env)))
        return rc;
    size_t whole = 0;
    for (int i = 0; i < n_horizons; ++i) {
        if (horizons[i] < 0 || horizons[i] > 1023)
            return fail(h, GRL_E_INVALID, "grl_trade_foresight: horizon " + std::to_string(i) + " is not 0 (the whole episode) or in 1..1023");
        whole += horizons[i] == 0 ? 1 : 0;
    }
    const int n = h->cfg.n_assets;
    const size_t cells = (size_t)max_steps * n * h->E;
    if (cells > TFS_MAX_PATH)
        return fail(h, GRL_E_INVALID, "grl_trade_foresight: max_steps * n_assets * E = " + std::to_string(cells) + " is over the limit of " +
                                          std::to_string(TFS_MAX_PATH) + " (2^28) path cells");
    if ((rc = trade_tape_check(h, fn, normals_host)) || (rc = episode_check_idle(h, fn))) return rc;
    hipSetDevice(h->cfg.device_id);
    TradeForesightState &w = h->tfs;
    w.n_horizons = 0;
    const size_t pairs = (size_t)n_horizons * h->E, trace = trace_env >= 0 ? (size_t)n_horizons * max_steps : 0;
    const size_t tape = normals_host ? cells : 0;
    if ((rc = episode_reserve(h, w.cap_h, n_horizons, {buf(w.horizons)})) ||
        (rc = episode_reserve(h, w.cap_pairs, pairs, {buf(w.final_assets), buf(w.bound), buf(w.trades), buf(w.depleted)}, &w.stats)) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_r), buf(w.trace_a), buf(w.trace_act, n)})) ||
        (rc = episode_reserve(h, w.cap_tape, tape, {buf(w.tape)})) || (rc = episode_reserve(h, w.cap_path, cells, {buf(w.path)})) ||
        (rc = episode_reserve(h, w.cap_dec, whole * cells, {buf(w.decisions)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.horizons, horizons, (size_t)n_horizons * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = trade_tape_upload(h, w.tape, normals_host, tape))) return rc;
    if (trace) {     // rows are defined up to the pair's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(w.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_a, 0, trace * 8, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_act, 0, trace * n * 4, h->stream));
    }
    const TradeParams R = trade_params(h);
    TradeForesightOut O{};
    O.stats = w.stats; O.final_assets = w.final_assets; O.bound = w.bound; O.trades = w.trades; O.depleted = w.depleted;
    O.trace_r = w.trace_r; O.trace_a = w.trace_a; O.trace_act = w.trace_act; O.dec = w.decisions;
    const bool path_only = trade_foresight_path_only();
    if ((rc = trade_foresight_launch(h, R, n_horizons, tape ? w.tape : nullptr, max_steps, trace_env, O, path_only)) || path_only) return rc;
    w.n_horizons = n_horizons; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_trade_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TradeForesightState &w = h->tfs;
    const size_t n = (size_t)h->cfg.n_assets;
    const size_t pairs = (size_t)w.n_horizons * h->E, trace = (size_t)w.n_horizons * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last call traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {
        {"final_assets", w.final_assets, pairs * 8}, {"bound", w.bound, pairs * 8}, {"trades", w.trades, pairs * 4},
        {"depleted", w.depleted, pairs}, {"prices", w.path, (size_t)w.max_steps * n * h->E * 8},
        {"trace_rewards", w.trace_r, trace * 4, untraced}, {"trace_assets", w.trace_a, trace * 8, untraced},
        {"trace_actions", w.trace_act, trace * n * 4, untraced}};
    return episode_read(h, "grl_trade_foresight_read", GRL_ENV_TRADE, "TradeAR1", w.n_horizons != 0, "grl_trade_foresight", outs, nullptr, which, host,
                        bytes, &w.stats, pairs);
}

}  // extern "C"
