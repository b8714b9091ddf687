// Optimal-savings yardstick for Solow at any order whose shock is Markov in m = max(p, q + 1) <= 4 numbers (C ABI:
// include/goldsrl_solowarmadp.h): backward induction on a (f_0, .., f_{m-1}, k) grid, f the forecasts of the ARMA(p, q) shock, one
// launch per stage, and the play of the tabulated policy, every env of the handle a whole episode in one launch.
//
// The split is trade_dp.hip's: the savings rate moves k and never f, so the expectation over the shock is the same for every k'
// a state can reach.  Solve, solow_arma_stage_kernel, a workgroup per exogenous node f:
//   1. nq * 2^m lanes place A f + b e_j on the f-axes: the corner offsets and weights go to LDS (240 at most).  They depend on
//      neither k nor the action, so a stage computes NX * nq * 2^m of them instead of NX * nk * ns * nq.
//   2. a lane per k contracts W[k] = sum_j w_j sum_corners wt * V_next[corner][k] into an LDS slab of nk doubles; k is the
//      fastest axis of the table, so every corner row is read coalesced.  Fixed order: nodes outer, corners ascending inner.
//   3. a wave per k node (4 per workgroup, striding over nk), lanes over the ns rates: Q = log((1 - s) y + 1e-4) + lerp(W, log k'),
//      two LDS reads in place of nq * 2^(m+1) global ones, then the wave arg-max of solow_dp_stage_kernel.
// The last stage has V_next = 0 and skips 1 and 2.  Everything is float64 and unfused, so that only exp / log / pow differ from the
// numpy restatement (tests/_solow_arma_dp_oracle.py).  The kernels take (A, b, Mz, Me) as data: p and q end on the host.
//
// Play, solow_arma_play_kernel: solow_dp_play_kernel's shape, one lane per env with the env's state in registers, the tape read a
// step ahead, solow_shock_next and solow_capital_step unchanged.  The action is the (m+1)-linear look-up at f = Mz zv + Me ev.
// The handle's state is read only; the error counter is the play's own.
#include <math.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"
#include "dp_axis.h"

namespace grl {

constexpr int AD_DIM = GRL_SOLOW_ARMA_DP_MAX_DIM;
constexpr int AD_LAGS = GRL_SOLOW_ARMA_DP_MAX_LAGS;
constexpr int AD_NQ = GRL_SOLOW_ARMA_DP_MAX_NODES;
constexpr int AD_CORNERS = AD_NQ << AD_DIM;                    // 240: fewer than the 256 lanes that place them
static_assert(AD_LAGS == 8, "the play keeps the lags in solow_shock_next's eight registers");

// the grid and what the host derives from it once
struct ArmaAxes {
    grl_solow_arma_dp_grid g;
    double lk_lo, dlk, ds, delta;
    double dx[AD_DIM];
    int stride[AD_DIM];                                         // of axis j, in exogenous nodes: axis m-1 is the fastest of them
    int m, NX;                                                  // NX: exogenous nodes, the product of nx[0..m-1]
};
// f' = A f + b eps
struct ArmaMove { double A[AD_DIM * AD_DIM], b[AD_DIM]; };
// f = mz zr + me er, the columns right-aligned like the lag registers of solow_shock_next
struct ArmaMap { double mz[AD_DIM][AD_LAGS], me[AD_DIM][AD_LAGS]; };

// One stage of the induction.  v_next: the value of the stage after it (not read when last), v_cur and policy: this stage's.
// Workgroup = one exogenous node; dynamic LDS: the slab, nk doubles.
__global__ __launch_bounds__(256) void solow_arma_stage_kernel(ArmaAxes X, ArmaMove M, const double *__restrict__ v_next,
                                                               double *__restrict__ v_cur, float *__restrict__ policy, int last) {
    extern __shared__ double arma_slab[];
    __shared__ int c_off[AD_CORNERS];
    __shared__ double c_wt[AD_CORNERS];
    __shared__ double q_wt[AD_NQ + 1];
    const grl_solow_arma_dp_grid &g = X.g;
    const int node = blockIdx.x, tid = threadIdx.x, m = X.m;
    double f[AD_DIM];
    int rest = node;
#pragma unroll
    for (int d = AD_DIM - 1; d >= 0; --d) {
        f[d] = 0.0;
        if (d < m) {
            f[d] = -g.x_max[d] + (double)(rest % g.nx[d]) * X.dx[d];
            rest /= g.nx[d];
        }
    }
    if (!last) {
        const int corners = 1 << m;
        if (tid < (g.nq << m)) {                               // step 1: corner c of node j
            const int j = tid >> m, c = tid & (corners - 1);
            double e = 0.0, w = 0.0;
#pragma unroll
            for (int i = 0; i < AD_NQ; ++i) if (i == j) { e = g.e_nodes[i]; w = g.e_weights[i]; }
            int off = 0;
            double wt = 1.0;
#pragma unroll
            for (int d = 0; d < AD_DIM; ++d) {
                if (d < m) {
                    double a = 0.0;
#pragma unroll
                    for (int l = 0; l < AD_DIM; ++l) if (l < m) a += M.A[d * AD_DIM + l] * f[l];
                    const DpCoord cd = dp_coord(a + M.b[d] * e, -g.x_max[d], X.dx[d], g.nx[d]);
                    const int bit = (c >> d) & 1;
                    off += (cd.i + bit) * X.stride[d];
                    wt *= bit ? cd.f : 1.0 - cd.f;
                }
            }
            c_off[tid] = off;
            c_wt[tid] = wt;
            if (c == 0) q_wt[j] = w;
        }
        __syncthreads();
        for (int ik = tid; ik < g.nk; ik += 256) {             // step 2
            double W = 0.0;
            for (int j = 0; j < g.nq; ++j) {
                double inner = 0.0;
                for (int c = 0; c < corners; ++c) {
                    const int e = (j << m) + c;
                    inner += c_wt[e] * v_next[(size_t)c_off[e] * g.nk + ik];
                }
                W += q_wt[j] * inner;
            }
            arma_slab[ik] = W;
        }
        __syncthreads();
    }
    const int lane = tid & 63;
    const double ez = exp(f[0]);
    for (int ik = tid >> 6; ik < g.nk; ik += 4) {              // step 3: wave-uniform ik
        const double k = exp(X.lk_lo + (double)ik * X.dlk);
        const double y = ez * pow(k, 0.33);
        double best = -__builtin_huge_val();
        int best_a = 0x7fffffff;
        for (int a = lane; a < g.ns; a += 64) {
            const double s = g.s_lo + (double)a * X.ds;
            const double r = log((1.0 - s) * y + 1e-4);
            double cont = 0.0;
            if (!last) {
                const double kn = (1.0 - X.delta) * k + s * y;
                const DpCoord ck = dp_coord(log(kn), X.lk_lo, X.dlk, g.nk);
                cont = (1.0 - ck.f) * arma_slab[ck.i] + ck.f * arma_slab[ck.i + 1];
            }
            const double q = r + cont;
            if (q > best) { best = q; best_a = a; }            // ascending a: the lowest index keeps a tie
        }
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const double oq = __shfl_xor(best, x);
            const int oa = __shfl_xor(best_a, x);
            if (oq > best || (oq == best && oa < best_a)) { best = oq; best_a = oa; }
        }
        if (lane == 0) {
            const size_t st = (size_t)node * g.nk + ik;
            v_cur[st] = best;
            policy[st] = (float)(g.s_lo + (double)best_a * X.ds);
        }
    }
}

struct ArmaPlayOut {
    PairStats stats;
    float *trace_a, *trace_r, *trace_k;
};

// the (m+1)-linear look-up of one stage's table at an env's float32 state: f, coordinates and blend in float64, rounded once.
// Corners of the f-axes ascending, bit d of the corner the upper neighbour on axis d; the blend in k innermost: 2^(m+1) loads.
__device__ __forceinline__ float arma_policy_action(const ArmaAxes &X, const ArmaMap &P, int p, int q, const float *__restrict__ tab,
                                                    float k, const float (&zr)[8], const float (&er)[8]) {
    const grl_solow_arma_dp_grid &g = X.g;
    const DpCoord ck = dp_coord(log((double)k), X.lk_lo, X.dlk, g.nk);
    DpCoord cx[AD_DIM];
#pragma unroll
    for (int d = 0; d < AD_DIM; ++d) {
        cx[d] = DpCoord{0, 0.0};
        if (d < X.m) {
            double f = 0.0;
#pragma unroll
            for (int j = 0; j < AD_LAGS; ++j) if (j >= AD_LAGS - p) f += P.mz[d][j] * (double)zr[j];
#pragma unroll
            for (int j = 0; j < AD_LAGS; ++j) if (j >= AD_LAGS - q) f += P.me[d][j] * (double)er[j];
            cx[d] = dp_coord(f, -g.x_max[d], X.dx[d], g.nx[d]);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < (1 << AD_DIM); ++c) {
        if (c < (1 << X.m)) {
            int off = 0;
            double wt = 1.0;
#pragma unroll
            for (int d = 0; d < AD_DIM; ++d) {
                if (d < X.m) {
                    const int bit = (c >> d) & 1;
                    off += (cx[d].i + bit) * X.stride[d];
                    wt *= bit ? cx[d].f : 1.0 - cx[d].f;
                }
            }
            const float *row = tab + (size_t)off * g.nk + ck.i;
            acc += wt * ((1.0 - ck.f) * (double)row[0] + ck.f * (double)row[1]);
        }
    }
    return (float)acc;
}

__global__ __launch_bounds__(64) void solow_arma_play_kernel(SolowParams S, SolowShockCoef C, ArmaAxes X, ArmaMap P, const float *__restrict__ policy,
                                                             int horizon, int max_steps, int trace_steps, ArmaPlayOut O) {
    const int env = blockIdx.x * 64 + threadIdx.x;          // a wave per workgroup: the waves spread over the CUs
    if (env >= S.E) return;
    const size_t E = S.E, n_states = (size_t)X.NX * X.g.nk;
    float k = S.k[env];
    RewardStats rs;
    float zr[8], er[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        zr[j] = j >= 8 - C.P ? S.z[(size_t)(j - (8 - C.P)) * E + env] : 0.f;
        er[j] = j >= 8 - C.Q ? S.e[(size_t)(j - (8 - C.Q)) * E + env] : 0.f;
    }
    const int pos0 = S.tape_pos[env], el0 = S.elapsed[env];
    int length = 0;
    bool finished = false;
    float e_t = pos0 >= 0 ? S.tape[(size_t)pos0 * E + env] : 0.f;
    for (int t = 0; t < max_steps; ++t) {
        const int pos = pos0 - t;
        if (pos < 0) {                                       // reference: IndexError, pop from empty list
            atomicAdd(S.err_flag, 1);
            break;
        }
        const float e_next = pos >= 1 ? S.tape[(size_t)(pos - 1) * E + env] : 0.f;     // next step's shock, asked for a step ahead
        int stage = S.max_steps > 0 ? horizon - (S.max_steps - (el0 + t)) : 0;
        stage = stage < 0 ? 0 : (stage > horizon - 1 ? horizon - 1 : stage);
        const float s = arma_policy_action(X, P, C.P, C.Q, policy + (size_t)stage * n_states, k, zr, er);
        const float ez = expf(zr[7]);
        const float rew = solow_capital_step(ez, S.delta, s, k);
        rs.add(rew);
        if (t < trace_steps) {
            const size_t o = (size_t)t * E + env;
            O.trace_a[o] = s; O.trace_r[o] = rew; O.trace_k[o] = k;
        }
        solow_shock_next(C, zr, er, e_t);
        e_t = e_next;
        length = t + 1;
        if (S.max_steps > 0 && el0 + length >= S.max_steps) { finished = true; break; }
    }
    O.stats.store(env, rs, length, finished);
}

// ---------------------------------------------------------------------------------------------- host
// The handle's model, in the operation order tests/_solow_arma_dp_oracle.py restates.  Lag l of the recursion is phi[l], th[l];
// the handle's arrays multiply the lags oldest first, so phi[l] = rho_z[p - l].
static int arma_model(grl_handle *h, const char *fn, grl_solow_arma_coef &M) {
    const std::string f(fn);
    if (h->cfg.env_kind != GRL_ENV_SOLOW) return fail(h, GRL_E_INVALID, f + ": not a Solow handle");
    const int p = h->so.P, q = h->so.Q, m = std::max(p, q + 1);
    if (h->cfg.solow_p < 1 || m > AD_DIM)
        return fail(h, GRL_E_INVALID, f + ": the handle has p = " + std::to_string(h->cfg.solow_p) + ", q = " + std::to_string(q) +
                                          ", so the shock's state has m = max(p, q + 1) = " + std::to_string(m) + " numbers; the grid covers p >= 1 and m <= 4");
    M = grl_solow_arma_coef{};
    M.m = m; M.p = p; M.q = q;
    double phi[AD_LAGS + 1] = {0}, th[AD_LAGS + 1] = {0};
    for (int l = 1; l <= p; ++l) phi[l] = (double)h->so.rho_z[p - l];
    for (int l = 1; l <= q; ++l) th[l] = (double)h->so.rho_e[q - l];
    M.b[0] = 1.0;
    for (int j = 1; j < m; ++j) {
        double a = th[j];
        for (int l = 1; l <= std::min(j, p); ++l) a += phi[l] * M.b[j - l];
        M.b[j] = a;
    }
    for (int j = 0; j + 1 < m; ++j) M.A[j * AD_DIM + j + 1] = 1.0;
    for (int l = 1; l <= p; ++l) M.A[(m - 1) * AD_DIM + (m - l)] = phi[l];
    // E_t[z_{t+j}] = sum_l phi_l E_t[z_{t+j-l}] + sum_{l >= j} th_l eps_{t+j-l}; a term at or before t is a lag of the env
    M.Mz[p - 1] = 1.0;
    for (int j = 1; j < m; ++j) {
        for (int i = 0; i < p; ++i) {
            double a = 0.0;
            for (int l = 1; l <= p; ++l) {
                if (j - l >= 0) a += phi[l] * M.Mz[(j - l) * AD_LAGS + i];
                else if (i == p - 1 - (l - j)) a += phi[l];
            }
            M.Mz[j * AD_LAGS + i] = a;
        }
        for (int i = 0; i < q; ++i) {
            double a = 0.0;
            for (int l = 1; l <= std::min(j, p); ++l) a += phi[l] * M.Me[(j - l) * AD_LAGS + i];
            for (int l = j; l <= q; ++l)
                if (i == q - 1 - (l - j)) a += th[l];
            M.Me[j * AD_LAGS + i] = a;
        }
    }
    double v[AD_DIM], acc[AD_DIM] = {0};
    for (int j = 0; j < AD_DIM; ++j) v[j] = M.b[j];
    for (int it = 0; it < 1024; ++it) {
        double nv[AD_DIM] = {0};
        for (int j = 0; j < m; ++j) {
            acc[j] += v[j] * v[j];
            double a = 0.0;
            for (int l = 0; l < m; ++l) a += M.A[j * AD_DIM + l] * v[l];
            nv[j] = a;
        }
        for (int j = 0; j < m; ++j) v[j] = nv[j];
    }
    for (int j = 0; j < m; ++j) M.f_std[j] = h->cfg.solow_sigma * sqrt(acc[j]);
    return GRL_OK;
}

static void arma_axes(const grl_solow_arma_dp_grid &g, int m, double delta, ArmaAxes &X) {
    X = ArmaAxes{};
    X.g = g;
    X.m = m;
    X.NX = 1;
    for (int d = m - 1; d >= 0; --d) {
        X.stride[d] = X.NX;
        X.NX *= g.nx[d];
        X.dx[d] = (g.x_max[d] + g.x_max[d]) / (double)(g.nx[d] - 1);
    }
    for (int d = m; d < AD_DIM; ++d) { X.g.nx[d] = 1; X.g.x_max[d] = 0.0; }
    for (int j = g.nq; j < AD_NQ; ++j) { X.g.e_nodes[j] = 0.0; X.g.e_weights[j] = 0.0; }
    X.lk_lo = log(g.k_lo);
    X.dlk = (log(g.k_hi) - X.lk_lo) / (double)(g.nk - 1);
    X.ds = (g.s_hi - g.s_lo) / (double)(g.ns - 1);
    X.delta = delta;
}

// the checks grl_solow_arma_dp_solve and grl_solow_arma_dp_set_policy share; fills M and X
static int arma_prepare(grl_handle *h, const char *fn, const grl_solow_arma_dp_grid *grid, int32_t horizon, grl_solow_arma_coef &M, ArmaAxes &X) {
    const std::string f(fn);
    int rc = arma_model(h, fn, M);
    if (rc) return rc;
    if (!grid) return fail(h, GRL_E_INVALID, f + ": null argument");
    if ((rc = episode_check_idle(h, fn))) return rc;
    const grl_solow_arma_dp_grid &g = *grid;
    if (g.nk < 2 || g.nk > GRL_SOLOW_ARMA_DP_MAX_NK || g.ns < 2 || g.ns > 65536)
        return fail(h, GRL_E_INVALID, f + ": needs 2 <= nk <= " + std::to_string(GRL_SOLOW_ARMA_DP_MAX_NK) + " and 2 <= ns <= 65536");
    if (g.nq < 1 || g.nq > AD_NQ) return fail(h, GRL_E_INVALID, f + ": nq must be in 1..15");
    if (horizon < 1) return fail(h, GRL_E_INVALID, f + ": horizon must be at least 1");
    if (!(g.k_lo > 0.0) || !(g.k_hi > g.k_lo) || !std::isfinite(g.k_hi)) return fail(h, GRL_E_INVALID, f + ": needs 0 < k_lo < k_hi");
    if (!(g.s_lo >= 0.0) || !(g.s_hi > g.s_lo) || !(g.s_hi <= 1.0)) return fail(h, GRL_E_INVALID, f + ": needs 0 <= s_lo < s_hi <= 1");
    const size_t most = GRL_SOLOW_ARMA_DP_MAX_TABLE_BYTES / 4 / (size_t)horizon;
    size_t n_states = (size_t)g.nk;
    bool over = false;
    for (int d = 0; d < M.m; ++d) {
        if (g.nx[d] < 2 || g.nx[d] > (1 << 20) || !(g.x_max[d] > 0.0) || !std::isfinite(g.x_max[d]))
            return fail(h, GRL_E_INVALID, f + ": needs 2 <= nx[j] <= 2^20 and x_max[j] > 0 on each of the m = " + std::to_string(M.m) + " axes");
        n_states *= (size_t)g.nx[d];                         // at most 2^12 * 2^20 * 2^28: no overflow before the cap is seen
        if (n_states > most) { over = true; n_states = most + 1; }
    }
    for (int j = 0; j < g.nq; ++j)
        if (!std::isfinite(g.e_nodes[j]) || !std::isfinite(g.e_weights[j])) return fail(h, GRL_E_INVALID, f + ": e_nodes and e_weights must be finite");
    if (over)
        return fail(h, GRL_E_SIZE, f + ": the policy table (horizon * nx[0] * .. * nx[m-1] * nk float32) would exceed " +
                                       std::to_string(GRL_SOLOW_ARMA_DP_MAX_TABLE_BYTES) + " bytes");
    arma_axes(g, M.m, h->cfg.solow_delta, X);
    return GRL_OK;
}

static int arma_grow_tables(grl_handle *h, size_t n_states, size_t table) {
    SolowArmaDpState &d = h->sad;
    const int rc = episode_reserve(h, d.cap_states, n_states, {buf(d.v[0]), buf(d.v[1])});
    return rc ? rc : episode_reserve(h, d.cap_table, table, {buf(d.policy)});
}

// nodes of the table the handle keeps (0 before the first)
static size_t arma_kept_states(const SolowArmaDpState &d, int m) {
    size_t n = d.horizon ? (size_t)d.grid.nk : 0;
    for (int j = 0; j < m; ++j) n *= (size_t)d.grid.nx[j];
    return n;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_solow_arma_model(grl_handle *h, grl_solow_arma_coef *model) {
    if (!h) return GRL_E_INVALID;
    grl_solow_arma_coef M;
    const int rc = arma_model(h, "grl_solow_arma_model", M);
    if (rc) return rc;
    if (!model) return fail(h, GRL_E_INVALID, "grl_solow_arma_model: null argument");
    *model = M;
    return GRL_OK;
}

int grl_solow_arma_dp_solve(grl_handle *h, const grl_solow_arma_dp_grid *grid, int32_t horizon) {
    if (!h) return GRL_E_INVALID;
    grl_solow_arma_coef M;
    ArmaAxes X;
    int rc = arma_prepare(h, "grl_solow_arma_dp_solve", grid, horizon, M, X);
    if (rc) return rc;
    hipSetDevice(h->cfg.device_id);
    SolowArmaDpState &d = h->sad;
    d.horizon = 0;
    const size_t n_states = (size_t)X.NX * X.g.nk;
    if ((rc = arma_grow_tables(h, n_states, (size_t)horizon * n_states))) return rc;
    ArmaMove mv;
    for (int i = 0; i < AD_DIM * AD_DIM; ++i) mv.A[i] = M.A[i];
    for (int i = 0; i < AD_DIM; ++i) mv.b[i] = M.b[i];
    const size_t lds = (size_t)X.g.nk * sizeof(double);
    rc = episode_launch(h, [&] {
        for (int t = horizon - 1; t >= 0; --t)
            hipLaunchKernelGGL(solow_arma_stage_kernel, dim3(X.NX), dim3(256), lds, h->stream, X, mv, d.v[(t + 1) & 1], d.v[t & 1],
                               d.policy + (size_t)t * n_states, t == horizon - 1 ? 1 : 0);
    });
    if (rc) return rc;
    d.grid = X.g; d.horizon = horizon; d.has_value = true;
    return GRL_OK;
}

int grl_solow_arma_dp_set_policy(grl_handle *h, const grl_solow_arma_dp_grid *grid, int32_t horizon, const float *policy_host) {
    if (!h) return GRL_E_INVALID;
    grl_solow_arma_coef M;
    ArmaAxes X;
    int rc = arma_prepare(h, "grl_solow_arma_dp_set_policy", grid, horizon, M, X);
    if (rc) return rc;
    if (!policy_host) return fail(h, GRL_E_INVALID, "grl_solow_arma_dp_set_policy: null argument");
    hipSetDevice(h->cfg.device_id);
    SolowArmaDpState &d = h->sad;
    d.horizon = 0;
    const size_t n_states = (size_t)X.NX * X.g.nk, table = (size_t)horizon * n_states;
    if ((rc = arma_grow_tables(h, n_states, table))) return rc;
    GRL_HIP(h, hipMemcpyAsync(d.policy, policy_host, table * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));              // the caller's array may go away
    d.grid = X.g; d.horizon = horizon; d.has_value = false;
    return GRL_OK;
}

int grl_solow_arma_dp_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowArmaDpState &d = h->sad;
    const size_t n_states = arma_kept_states(d, std::max(h->so.P, h->so.Q + 1));
    const EpisodeOut outs[] = {
        {"policy", d.policy, (size_t)d.horizon * n_states * 4},
        {"value", d.v[0], n_states * 8, d.has_value ? nullptr : "the table was set, not solved: it has no value function"}};
    return episode_read(h, "grl_solow_arma_dp_read", GRL_ENV_SOLOW, "Solow", d.horizon != 0, "grl_solow_arma_dp_solve or grl_solow_arma_dp_set_policy",
                        outs, nullptr, which, host, bytes);
}

int grl_solow_arma_dp_play(grl_handle *h, int32_t max_steps, int32_t trace_steps) {
    const char *fn = "grl_solow_arma_dp_play";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SOLOW, "Solow", true)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    if (trace_steps < 0 || trace_steps > max_steps) return fail(h, GRL_E_INVALID, "grl_solow_arma_dp_play: trace_steps must be in 0..max_steps");
    if ((rc = episode_check_idle(h, fn))) return rc;
    SolowArmaDpState &d = h->sad;
    if (d.horizon == 0) return fail(h, GRL_E_STATE, "grl_solow_arma_dp_play: call grl_solow_arma_dp_solve or grl_solow_arma_dp_set_policy first");
    grl_solow_arma_coef M;                                   // a table exists, so the handle has a model
    if ((rc = arma_model(h, fn, M))) return rc;
    hipSetDevice(h->cfg.device_id);
    d.played = 0;
    const size_t envs = h->E, trace = (size_t)trace_steps * envs;
    if ((!d.err && (rc = grow(h, &d.err, 1))) ||
        (rc = episode_reserve(h, d.cap_envs, envs, {}, &d.stats)) ||
        (rc = episode_reserve(h, d.cap_trace, trace, {buf(d.trace_a), buf(d.trace_r), buf(d.trace_k)})))
        return rc;
    GRL_HIP(h, hipMemsetAsync(d.err, 0, 4, h->stream));
    if (trace) {     // rows are defined up to the env's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(d.trace_a, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(d.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(d.trace_k, 0, trace * 4, h->stream));
    }
    SolowParams S = solow_params(h);
    S.err_flag = d.err;
    const SolowShockCoef C = solow_shock_coef(S);
    ArmaAxes X;
    arma_axes(d.grid, M.m, h->cfg.solow_delta, X);
    ArmaMap P{};
    for (int j = 0; j < M.m; ++j) {
        for (int i = 0; i < M.p; ++i) P.mz[j][AD_LAGS - M.p + i] = M.Mz[j * AD_LAGS + i];
        for (int i = 0; i < M.q; ++i) P.me[j][AD_LAGS - M.q + i] = M.Me[j * AD_LAGS + i];
    }
    ArmaPlayOut O{};
    O.stats = d.stats; O.trace_a = d.trace_a; O.trace_r = d.trace_r; O.trace_k = d.trace_k;
    rc = episode_launch(h, [&] {
        hipLaunchKernelGGL(solow_arma_play_kernel, dim3((h->E + 63) / 64), dim3(64), 0, h->stream, S, C, X, P, d.policy, d.horizon, max_steps, trace_steps, O);
    });
    if (rc) return rc;
    d.played = h->E; d.trace_steps = trace_steps;
    return GRL_OK;
}

int grl_solow_arma_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowArmaDpState &d = h->sad;
    const size_t envs = h->E, trace = (size_t)d.trace_steps * envs;
    const char *untraced = d.trace_steps == 0 ? "the last play kept no trace (trace_steps was 0)" : nullptr;
    const EpisodeOut outs[] = {
        {"actions", d.trace_a, trace * 4, untraced}, {"rewards", d.trace_r, trace * 4, untraced}, {"k", d.trace_k, trace * 4, untraced}};
    return episode_read(h, "grl_solow_arma_dp_play_read", GRL_ENV_SOLOW, "Solow", d.played != 0, "grl_solow_arma_dp_play", outs, d.err, which, host, bytes,
                        &d.stats, envs);
}

}  // extern "C"
