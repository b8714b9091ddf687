// Attainable optimum of TradeAR1 (C ABI: include/goldsrl_tradedp.h, where the model is written out): backward induction over
// non-anticipating policies on a (shares, log prices) grid, one launch per stage, and the play of the tabulated policy, every env
// of the handle a whole episode in one launch.
//
// Solve, trade_dp_stage_kernel<N>: ONE WORKGROUP PER PRICE NODE.  From a price node the next prices x' = 0.9 x + e_k depend on the
// quadrature node alone, not on the action or the shares, so the price half of the 2n-linear look-up of V_j is the same for every
// (share node, action) of the workgroup.
//   setup    lanes 0 .. n * nq - 1: exp(x'_a - x_a) and the x-coordinate of x'_a per (asset, node) into LDS; the weights beside them.
//   phase 1  the workgroup contracts the price axes of V_j into the slab S[k_0][k_1][u_0][u_1], nq^n * nu^n doubles of LDS, 2^n
//            global reads per entry.  V is kept [price node][share node] between the stages, so consecutive lanes read consecutive
//            doubles; the top stage's value is also stored [share node][price node], the layout it is read in.
//   phase 2  after one barrier each wave takes share nodes in turn and its lanes stride over the na^n joint actions; per joint
//            quadrature node a lane computes g, u'' and an n-linear look-up in S: 2^n LDS reads where a gather from V would be 4^n
//            global ones.  log g is the only transcendental of the inner loop.
//   arg-max  a wave reduction on (Q, lowest joint index); lane 0 stores the value and the n float32 action components.
// Everything is float64 and, like the rest of the library, unfused: one IEEE operation per statement, sums in the order the
// header states, so that only exp / log differ from the numpy restatement (tests/_trade_dp_oracle.py).  No workgroup talks to
// another; the stages are ordered by the stream.
//
// Play, trade_dp_play_kernel<N>: one lane per env with the account in registers, the step loop of trade_sweep_play
// (trade_sweep_dev.h) with the table's action in place of a rule's: trade_asset_trade, trade_account_settle and trade_prices_step
// of flat_env_dev.h, unchanged and in that order.  The handle's state is read only: nothing here writes cash, assets, q, p, nstep,
// elapsed, the outputs, the done list or the episode records.
#include <math.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"
#include "trade_dp_lookup.h"      // the table's look-up, shared with the grid trader's teacher

namespace grl {

constexpr int TDP_NQ = GRL_TRADE_DP_MAX_NODES;
constexpr int TDP_THREADS = 512;                 // 8 waves: two per SIMD, 256 registers each

// the grid and what the host derives from it once
struct TdpArgs {
    grl_trade_dp_grid g;
    double um1;                                  // nu - 1: u = i / um1, the coordinate of u is u * um1
    double am1;                                  // na - 1: a = (2 i - (na - 1)) / am1
    double dx;                                   // (x_max + x_max) / (nx - 1)
    int n, NU, NX, NA, NK;                       // nu^n, nx^n, na^n, nq^n
};

// component i of the action grid: exactly -1, 0 and 1 at the ends and the middle
__device__ __forceinline__ double tdp_action(int i, int na, double am1) { return (double)(2 * i - (na - 1)) / am1; }

// the share after the trade, on the cash share c the step began with
__device__ __forceinline__ double tdp_share_move(double u, double a, double c, double nd) {
    if (a > 0.0) {
        double t = a / nd;
        t = t * c;
        return u + t;
    }
    const double m = 1.0 + a;
    return u * m;
}

// One stage: v_next is V_j [price node][share node], v_cur V_{j+1} in the same layout, value V_{j+1} [share node][price node],
// policy row j.  Dynamic LDS: S (NK * NU doubles), R and the x-fractions (N * nq each), the weights (nq), the x-indices (N * nq
// ints).
template <int N>
__global__ __launch_bounds__(TDP_THREADS) void trade_dp_stage_kernel(TdpArgs A, const double *__restrict__ v_next, double *__restrict__ v_cur,
                                                                     double *__restrict__ value, float *__restrict__ policy) {
    extern __shared__ double tdp_lds[];
    const grl_trade_dp_grid &g = A.g;
    const int nq = g.nq, nu = g.nu, nx = g.nx, na = g.na, NU = A.NU;
    double *S = tdp_lds;
    double *Rr = S + (size_t)A.NK * NU;
    double *fx = Rr + N * nq;
    double *wq = fx + N * nq;
    int *ixn = (int *)(wq + nq);
    const int xn = blockIdx.x;                                 // the workgroup's price node
    const int tid = threadIdx.x;

    if (tid < N * nq) {
        const int a = tid / nq, k = tid - a * nq;
        const int ix = N == 1 ? xn : (a == 0 ? xn / nx : xn % nx);
        double e = 0.0, w = 0.0;
#pragma unroll
        for (int j = 0; j < TDP_NQ; ++j) if (j == k) { e = g.e_nodes[j]; w = g.e_weights[j]; }
        const double off = (double)ix * A.dx;
        const double x = -g.x_max + off;
        const double m = 0.9 * x;
        const double xp = m + e;
        const double d = xp - x;
        Rr[tid] = exp(d);
        const double s = xp + g.x_max;
        const TdpCoord c = tdp_coord(s / A.dx, nx);
        ixn[tid] = c.i; fx[tid] = c.f;
        if (a == 0) wq[k] = w;
    }
    __syncthreads();

    // phase 1: the price axes of V_j, once for the workgroup
    for (int e = tid; e < A.NK * NU; e += TDP_THREADS) {
        const int k = e / NU, s = e - k * NU;
        if constexpr (N == 1) {
            const size_t o = (size_t)ixn[k] * NU + s;
            S[e] = tdp_lerp(fx[k], v_next[o], v_next[o + NU]);
        } else {
            const int k0 = k / nq, k1 = nq + (k - k0 * nq);
            const size_t o = ((size_t)ixn[k0] * nx + ixn[k1]) * NU + s, d0 = (size_t)nx * NU;
            const double v0 = tdp_lerp(fx[k1], v_next[o], v_next[o + NU]);
            const double v1 = tdp_lerp(fx[k1], v_next[o + d0], v_next[o + d0 + NU]);
            S[e] = tdp_lerp(fx[k0], v0, v1);
        }
    }
    __syncthreads();

    // phase 2: a wave per share node, lanes over the joint actions
    const int lane = tid & 63;
    const double nd = (double)N;
    for (int s = tid >> 6; s < NU; s += TDP_THREADS / 64) {       // wave-uniform
        double u0, u1 = 0.0;
        if constexpr (N == 1) {
            u0 = (double)s / A.um1;
        } else {
            const int i0 = s / nu;
            u0 = (double)i0 / A.um1;
            u1 = (double)(s - i0 * nu) / A.um1;
            const double sum = u0 + u1;
            if (sum > 1.0) { u0 = u0 / sum; u1 = u1 / sum; }  // the node stands for the state on the simplex's face
        }
        double c = 1.0 - u0;
        if constexpr (N == 2) c = c - u1;

        double best = -__builtin_huge_val();
        int best_a = 0x7fffffff;
        for (int ja = lane; ja < A.NA; ja += 64) {
            const int j0 = N == 1 ? ja : ja / na;
            const double up0 = tdp_share_move(u0, tdp_action(j0, na, A.am1), c, nd);
            double up1 = 0.0;
            if constexpr (N == 2) up1 = tdp_share_move(u1, tdp_action(ja - j0 * na, na, A.am1), c, nd);
            double cp = 1.0 - up0;
            if constexpr (N == 2) cp = cp - up1;
            double acc = 0.0;
            for (int k0 = 0; k0 < nq; ++k0) {
                const double y0 = up0 * Rr[k0];
                if constexpr (N == 1) {
                    const double gr = cp + y0;
                    const double un0 = y0 / gr;
                    const TdpCoord c0 = tdp_coord(un0 * A.um1, nu);
                    const double *Sk = S + (size_t)k0 * NU + c0.i;
                    const double v = tdp_lerp(c0.f, Sk[0], Sk[1]);
                    const double term = log(gr) + v;
                    const double wt = wq[k0] * term;
                    acc = acc + wt;
                } else {
                    for (int k1 = 0; k1 < nq; ++k1) {
                        const double y1 = up1 * Rr[nq + k1];
                        double gr = cp + y0;
                        gr = gr + y1;
                        const double un0 = y0 / gr;
                        const double un1 = y1 / gr;
                        const TdpCoord c0 = tdp_coord(un0 * A.um1, nu), c1 = tdp_coord(un1 * A.um1, nu);
                        const double *Sk = S + (size_t)(k0 * nq + k1) * NU + c0.i * nu + c1.i;
                        const double v0 = tdp_lerp(c1.f, Sk[0], Sk[1]);
                        const double v1 = tdp_lerp(c1.f, Sk[nu], Sk[nu + 1]);
                        const double v = tdp_lerp(c0.f, v0, v1);
                        const double term = log(gr) + v;
                        const double wk = wq[k0] * wq[k1];
                        const double wt = wk * term;
                        acc = acc + wt;
                    }
                }
            }
            if (acc > best) { best = acc; best_a = ja; }       // ascending ja: the lowest index keeps a tie
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double oq = __shfl_xor(best, m);
            const int oa = __shfl_xor(best_a, m);
            if (oq > best || (oq == best && oa < best_a)) { best = oq; best_a = oa; }
        }
        if (lane == 0) {
            if (best_a >= A.NA) best_a = 0;                    // every Q was NaN: hold
            const size_t st = (size_t)s * A.NX + xn;
            v_cur[(size_t)xn * NU + s] = best;
            value[st] = best;
            if constexpr (N == 1) {
                policy[st] = (float)tdp_action(best_a, na, A.am1);
            } else {
                const int j0 = best_a / na;
                policy[st * 2] = (float)tdp_action(j0, na, A.am1);
                policy[st * 2 + 1] = (float)tdp_action(best_a - j0 * na, na, A.am1);
            }
        }
    }
}

struct TdpPlayOut {
    PairStats stats;
    double *final_assets, *trace_a;
    uint8_t *depleted;
    float *trace_act, *trace_r;
};

template <int N>
__global__ __launch_bounds__(64) void trade_dp_play_kernel(TradeParams R_, TdpAxes A, const float *__restrict__ policy, int horizon,
                                                            const float *__restrict__ tape, int max_steps, int trace_steps, TdpPlayOut O) {
    const int env = blockIdx.x * 64 + threadIdx.x;          // a wave per workgroup: the waves spread over the CUs
    TradeParams R = R_;
    R.n = N;                                                 // the host launches <n_assets>: the unused slot's code folds away
    if (env >= R.E) return;
    const size_t E = R.E;
    double cash = R.cash[env], assets = R.assets[env];
    double p[2] = {1.0, 1.0}, q[2] = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < N; ++a) { p[a] = R.p[a * E + env]; q[a] = R.q[a * E + env]; }
    const uint32_t st0 = R.nstep[env];
    const int el0 = R.elapsed[env];
    RewardStats rs;
    int length = 0;
    bool finished = false, depleted = false;
    for (int t = 0; t < max_steps; ++t) {
        const bool last = R.max_steps > 0 && el0 + t + 1 >= R.max_steps;
        float act[2];
        tdp_lookup<N>(A, policy, horizon, tdp_moves(R.max_steps, el0 + t, horizon), cash, q, p, act);      // trade_dp_lookup.h
        double cost = 0.0, value = 0.0;
        const double c0 = cash;
#pragma unroll
        for (int a = 0; a < N; ++a) trade_asset_trade(act[a], R.n, c0, p[a], q[a], cost, value);
        bool dep;
        const float rew = trade_account_settle(cash, assets, cost, value, dep);
        rs.add(rew);
        length = t + 1;
        if (t < trace_steps) {
            const size_t o = (size_t)t * E + env;
            O.trace_r[o] = rew; O.trace_a[o] = assets;
#pragma unroll
            for (int a = 0; a < N; ++a) O.trace_act[((size_t)t * N + a) * E + env] = act[a];
        }
        depleted = dep;
        finished = dep || last;
        if (finished || t + 1 == max_steps) break;
        trade_prices_step<2>(R, tape, env, st0, t, 1, [&](int a) { return a < N ? p[a] : 1.0; }, [&](int a, double v) { if (a < N) p[a] = v; });
    }
    O.stats.store(env, rs, length, finished);
    O.final_assets[env] = assets; O.depleted[env] = depleted ? 1 : 0;
}

static size_t tdp_pow(int base, int n) { return n == 1 ? (size_t)base : (size_t)base * base; }

static size_t tdp_lds_bytes(const TdpArgs &A) {
    const size_t nq = A.g.nq, n = A.n;
    return ((size_t)A.NK * A.NU + 2 * n * nq + nq) * sizeof(double) + ((n * nq * sizeof(int) + 7) & ~(size_t)7);
}

// the checks grl_trade_dp_solve and grl_trade_dp_set_policy share; fills A.  solve: the slab must fit too
static int tdp_prepare(grl_handle *h, const char *fn, const grl_trade_dp_grid *grid, int32_t horizon, bool solve, TdpArgs &A) {
    const std::string f(fn);
    if (h->cfg.env_kind != GRL_ENV_TRADE) return fail(h, GRL_E_INVALID, f + ": not a TradeAR1 handle");
    const int n = h->cfg.n_assets;
    if (n > 2)
        return fail(h, GRL_E_INVALID, f + ": the handle has n_assets = " + std::to_string(n) +
                                          "; the grid covers n_assets 1 and 2 (it grows by two dimensions per asset)");
    if (!grid) return fail(h, GRL_E_INVALID, f + ": null argument");
    if (h->step_in_flight) return fail(h, GRL_E_INVALID, f + ": a step is in flight (grl_wait first)");
    const grl_trade_dp_grid &g = *grid;
    if (g.nu < 2 || g.nx < 2 || g.nu > 16384 || g.nx > 16384) return fail(h, GRL_E_INVALID, f + ": nu and nx must be in 2..16384");
    if (g.na < 3 || g.na > 4095 || g.na % 2 == 0) return fail(h, GRL_E_INVALID, f + ": na must be odd (0 is an action) and in 3..4095");
    if (g.nq < 1 || g.nq > TDP_NQ) return fail(h, GRL_E_INVALID, f + ": nq must be in 1..15");
    if (horizon < 1) return fail(h, GRL_E_INVALID, f + ": horizon must be at least 1");
    if (!(g.x_max > 0.0) || !std::isfinite(g.x_max)) return fail(h, GRL_E_INVALID, f + ": needs x_max > 0");
    for (int j = 0; j < g.nq; ++j) {
        if (!std::isfinite(g.e_nodes[j]) || !std::isfinite(g.e_weights[j]) || (j > 0 && !(g.e_nodes[j] > g.e_nodes[j - 1])))
            return fail(h, GRL_E_INVALID, f + ": e_nodes must be finite and ascending, e_weights finite");
    }
    A = TdpArgs{};
    A.g = g;
    for (int j = g.nq; j < TDP_NQ; ++j) { A.g.e_nodes[j] = 0.0; A.g.e_weights[j] = 0.0; }
    A.n = n;
    const size_t NU = tdp_pow(g.nu, n), NX = tdp_pow(g.nx, n);
    A.NK = (int)tdp_pow(g.nq, n); A.NA = (int)tdp_pow(g.na, n);
    A.um1 = (double)(g.nu - 1); A.am1 = (double)(g.na - 1);
    A.dx = (g.x_max + g.x_max) / (double)(g.nx - 1);
    if (solve) {
        const size_t slab = (size_t)A.NK * NU * sizeof(double);
        A.NU = (int)NU;
        if (slab > GRL_TRADE_DP_MAX_LDS_BYTES || tdp_lds_bytes(A) > GRL_TRADE_DP_MAX_LDS_BYTES)
            return fail(h, GRL_E_SIZE, f + ": the slab of nq^n * nu^n float64 (nq = " + std::to_string(g.nq) + ", nu = " + std::to_string(g.nu) +
                                           ", n = " + std::to_string(n) + ": " + std::to_string(slab) + " bytes) does not fit the " +
                                           std::to_string(GRL_TRADE_DP_MAX_LDS_BYTES) + " bytes of LDS a workgroup can have");
    }
    if (NU * NX > GRL_TRADE_DP_MAX_TABLE_BYTES / 4 / (size_t)n / (size_t)horizon)
        return fail(h, GRL_E_SIZE, f + ": the policy table (horizon * nu^n * nx^n * n float32 = " + std::to_string(horizon) + " * " +
                                       std::to_string(NU) + " * " + std::to_string(NX) + " * " + std::to_string(n) + " * 4 bytes) would exceed " +
                                       std::to_string(GRL_TRADE_DP_MAX_TABLE_BYTES) + " bytes");
    A.NU = (int)NU; A.NX = (int)NX;
    return GRL_OK;
}

static int tdp_grow_tables(grl_handle *h, size_t n_states, size_t table) {
    TradeDpState &d = h->tdp;
    const int rc = episode_reserve(h, d.cap_states, n_states, {buf(d.v[0]), buf(d.v[1]), buf(d.value)});
    return rc ? rc : episode_reserve(h, d.cap_table, table, {buf(d.policy)});
}

template <int N>
static int tdp_launch_stages(grl_handle *h, const TdpArgs &A, int horizon) {
    TradeDpState &d = h->tdp;
    const size_t lds = tdp_lds_bytes(A), NS = (size_t)A.NU * A.NX;
    GRL_HIP(h, hipFuncSetAttribute((const void *)trade_dp_stage_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRL_TRADE_DP_MAX_LDS_BYTES));
    GRL_HIP(h, hipMemsetAsync(d.v[0], 0, NS * sizeof(double), h->stream));               // V_0 = 0
    return episode_launch(h, [&] {
        for (int j = 0; j < horizon; ++j)
            hipLaunchKernelGGL(trade_dp_stage_kernel<N>, dim3(A.NX), dim3(TDP_THREADS), lds, h->stream, A, d.v[j & 1], d.v[(j + 1) & 1], d.value,
                               d.policy + (size_t)j * NS * N);
    });
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_trade_dp_solve(grl_handle *h, const grl_trade_dp_grid *grid, int32_t horizon) {
    if (!h) return GRL_E_INVALID;
    TdpArgs A;
    int rc = tdp_prepare(h, "grl_trade_dp_solve", grid, horizon, true, A);
    if (rc) return rc;
    hipSetDevice(h->cfg.device_id);
    TradeDpState &d = h->tdp;
    d.horizon = 0;
    const size_t NS = (size_t)A.NU * A.NX;
    if ((rc = tdp_grow_tables(h, NS, (size_t)horizon * NS * A.n))) return rc;
    rc = A.n == 1 ? tdp_launch_stages<1>(h, A, horizon) : tdp_launch_stages<2>(h, A, horizon);
    if (rc) return rc;
    d.grid = A.g; d.horizon = horizon; d.has_value = true;
    return GRL_OK;
}

int grl_trade_dp_set_policy(grl_handle *h, const grl_trade_dp_grid *grid, int32_t horizon, const float *policy_host) {
    if (!h) return GRL_E_INVALID;
    TdpArgs A;
    int rc = tdp_prepare(h, "grl_trade_dp_set_policy", grid, horizon, false, A);
    if (rc) return rc;
    if (!policy_host) return fail(h, GRL_E_INVALID, "grl_trade_dp_set_policy: null argument");
    hipSetDevice(h->cfg.device_id);
    TradeDpState &d = h->tdp;
    d.horizon = 0;
    const size_t NS = (size_t)A.NU * A.NX, table = (size_t)horizon * NS * A.n;
    if ((rc = tdp_grow_tables(h, NS, table))) return rc;
    GRL_HIP(h, hipMemcpyAsync(d.policy, policy_host, table * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));              // the caller's array may go away
    d.grid = A.g; d.horizon = horizon; d.has_value = false;
    return GRL_OK;
}

int grl_trade_dp_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TradeDpState &d = h->tdp;
    const int n = h->cfg.n_assets > 2 ? 1 : h->cfg.n_assets;
    const size_t NS = d.horizon ? tdp_pow(d.grid.nu, n) * tdp_pow(d.grid.nx, n) : 0;
    const EpisodeOut outs[] = {
        {"policy", d.policy, (size_t)d.horizon * NS * n * 4},
        {"value", d.value, NS * 8, d.has_value ? nullptr : "the table was set, not solved: it has no value function"}};
    return episode_read(h, "grl_trade_dp_read", GRL_ENV_TRADE, "TradeAR1", d.horizon != 0, "grl_trade_dp_solve or grl_trade_dp_set_policy", outs, nullptr,
                        which, host, bytes);
}

int grl_trade_dp_play(grl_handle *h, const float *normals_host, int32_t max_steps, int32_t trace_steps) {
    const char *fn = "grl_trade_dp_play";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TRADE, "TradeAR1", true)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    if (trace_steps < 0 || trace_steps > max_steps) return fail(h, GRL_E_INVALID, "grl_trade_dp_play: trace_steps must be in 0..max_steps");
    if ((rc = trade_tape_check(h, fn, normals_host)) || (rc = episode_check_idle(h, fn))) return rc;
    TradeDpState &d = h->tdp;
    if (d.horizon == 0) return fail(h, GRL_E_STATE, "grl_trade_dp_play: call grl_trade_dp_solve or grl_trade_dp_set_policy first");
    hipSetDevice(h->cfg.device_id);
    d.played = 0;
    const int n = h->cfg.n_assets;                            // 1 or 2: a table exists
    const size_t envs = h->E, trace = (size_t)trace_steps * envs;
    const size_t tape = normals_host ? (size_t)max_steps * n * envs : 0;
    if ((rc = episode_reserve(h, d.cap_envs, envs, {buf(d.final_assets), buf(d.depleted)}, &d.stats)) ||
        (rc = episode_reserve(h, d.cap_trace, trace, {buf(d.trace_act, 2), buf(d.trace_r), buf(d.trace_a)})) ||
        (rc = episode_reserve(h, d.cap_tape, tape, {buf(d.tape)})))
        return rc;
    if ((rc = trade_tape_upload(h, d.tape, normals_host, tape))) return rc;
    if (trace) {     // rows are defined up to the env's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(d.trace_act, 0, trace * n * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(d.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(d.trace_a, 0, trace * 8, h->stream));
    }
    const TradeParams R = trade_params(h);
    const TdpAxes A = tdp_axes(d.grid, n);
    TdpPlayOut O{};
    O.stats = d.stats; O.final_assets = d.final_assets; O.depleted = d.depleted;
    O.trace_act = d.trace_act; O.trace_r = d.trace_r; O.trace_a = d.trace_a;
    const float *tp = tape ? d.tape : nullptr;
    const dim3 grid_dim((h->E + 63) / 64), block(64);
    rc = episode_launch(h, [&] {
        if (n == 1) hipLaunchKernelGGL(trade_dp_play_kernel<1>, grid_dim, block, 0, h->stream, R, A, d.policy, d.horizon, tp, max_steps, trace_steps, O);
        else hipLaunchKernelGGL(trade_dp_play_kernel<2>, grid_dim, block, 0, h->stream, R, A, d.policy, d.horizon, tp, max_steps, trace_steps, O);
    });
    if (rc) return rc;
    d.played = h->E; d.trace_steps = trace_steps;
    return GRL_OK;
}

int grl_trade_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TradeDpState &d = h->tdp;
    const size_t envs = h->E, trace = (size_t)d.trace_steps * envs;
    const char *untraced = d.trace_steps == 0 ? "the last play kept no trace (trace_steps was 0)" : nullptr;
    const EpisodeOut outs[] = {
        {"final_assets", d.final_assets, envs * 8}, {"depleted", d.depleted, envs},
        {"actions", d.trace_act, trace * h->cfg.n_assets * 4, untraced}, {"rewards", d.trace_r, trace * 4, untraced}, {"assets", d.trace_a, trace * 8, untraced}};
    return episode_read(h, "grl_trade_dp_play_read", GRL_ENV_TRADE, "TradeAR1", d.played != 0, "grl_trade_dp_play", outs, nullptr, which, host, bytes, &d.stats, envs);
}

}  // extern "C"
