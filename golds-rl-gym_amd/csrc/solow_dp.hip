// Optimal-savings yardstick for Solow (C ABI: include/goldsrl_solowdp.h): backward induction on a (k, z, e) grid, one launch per
// stage, and the play of the tabulated policy, every env of the handle a whole episode in one launch.
//
// Solve, solow_dp_stage_kernel: one wave per state, lanes over actions, a wave arg-max.  A state's share -- exp(z), k^alpha and
// the nq look-up rows in z, which do not depend on the action -- is computed once per wave (every lane holds it, the wave's time is
// one lane's); an action's share is two logs and nq bilinear look-ups into V_next, which stays in L1 / L2 (134 KB at the default
// grid).  Measured against a lane per state looping over the actions: 13.7 ms against 39.2 ms for the default solve (96 x 25 x 7,
// 96 actions, 256 stages), 0.84 against 5.0 ms at 32 x 9 x 3 (LABNOTES.md) -- 16 800 states are 263 waves, one per CU, each
// a chain of 96 dependent steps.  No workgroup talks to another; the stages are ordered by the stream.  Everything is float64 and, like the rest of the
// library, unfused, so that only exp / log / pow differ from a numpy restatement (tests/_solow_dp_oracle.py).
//
// Play, solow_dp_play_kernel: one lane per env with the env's state in registers, the shape of solow_sweep_kernel: the shock
// recursion is solow_shock_next, the step solow_capital_step, the tape is read a step ahead.  The handle's state is read only:
// nothing here writes k, z, e, tape_pos, elapsed, the outputs or the episode records, and the error counter is the play's own.
#include <math.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"

namespace grl {

constexpr int DP_NQ = GRL_SOLOW_DP_MAX_NODES;

// the grid and what the host derives from it once: log k_lo, the three steps, the model
struct DpArgs {
    grl_solow_dp_grid g;
    double lk_lo, dlk, dz, ds;
    double rho, theta, delta;
    int ne, n_states;
};

// position on a uniform axis of n points from lo in steps of `step`, clamped to the axis: the lower neighbour and the share of
// the upper one.  A NaN lands on point 0, so the index is always inside the table.
struct DpCoord { int i; double f; };
__device__ __forceinline__ DpCoord dp_coord(double x, double lo, double step, int n) {
    double u = (x - lo) / step;
    u = fmin(fmax(u, 0.0), (double)(n - 1));
    int i = (int)u;
    if (i > n - 2) i = n - 2;
    return DpCoord{i, u - (double)i};
}

// bilinear look-up in the (k, z) plane `je` of a row-major (nk, nz, ne) table
template <typename T>
__device__ __forceinline__ double dp_bilinear(const T *__restrict__ tab, int nz, int ne, DpCoord ck, DpCoord cz, int je) {
    const size_t o = ((size_t)ck.i * nz + cz.i) * ne + je, dk = (size_t)nz * ne;
    const double v00 = (double)tab[o], v10 = (double)tab[o + dk], v01 = (double)tab[o + ne], v11 = (double)tab[o + dk + ne];
    const double v0 = (1.0 - ck.f) * v00 + ck.f * v10;
    const double v1 = (1.0 - ck.f) * v01 + ck.f * v11;
    return (1.0 - cz.f) * v0 + cz.f * v1;
}

// One stage of the induction.  v_next: the value of the stage after it (not read when last), v_cur and policy: this stage's.
// Workgroup = 4 waves = 4 states; lane l of a wave takes the actions l, l + 64, ...
__global__ __launch_bounds__(256) void solow_dp_stage_kernel(DpArgs A, const double *__restrict__ v_next, double *__restrict__ v_cur,
                                                             float *__restrict__ policy, int last) {
    const int lane = threadIdx.x & 63;
    const int st = blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (st >= A.n_states) return;
    const grl_solow_dp_grid &g = A.g;
    const int ie = st % A.ne, iz = (st / A.ne) % g.nz, ik = st / (A.ne * g.nz);
    const double k = exp(A.lk_lo + (double)ik * A.dlk);
    const double z = -g.z_max + (double)iz * A.dz;
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < DP_NQ; ++j) if (j == ie) e = g.e_nodes[j];
    const double y = exp(z) * pow(k, 0.33);
    const double zc = A.rho * z + A.theta * e;
    DpCoord cz[DP_NQ];
#pragma unroll
    for (int j = 0; j < DP_NQ; ++j) cz[j] = j < g.nq ? dp_coord(zc + g.e_nodes[j], -g.z_max, A.dz, g.nz) : DpCoord{0, 0.0};

    double best = -__builtin_huge_val();
    int best_a = 0x7fffffff;
    for (int a = lane; a < g.ns; a += 64) {
        const double s = g.s_lo + (double)a * A.ds;
        const double r = log((1.0 - s) * y + 1e-4);
        double acc = 0.0;
        if (!last) {
            const double kn = (1.0 - A.delta) * k + s * y;
            const DpCoord ck = dp_coord(log(kn), A.lk_lo, A.dlk, g.nk);
#pragma unroll
            for (int j = 0; j < DP_NQ; ++j)
                if (j < g.nq) acc += g.e_weights[j] * dp_bilinear(v_next, g.nz, A.ne, ck, cz[j], A.ne > 1 ? j : 0);
        }
        const double q = r + acc;
        if (q > best) { best = q; best_a = a; }              // ascending a: the lowest index keeps a tie
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oq = __shfl_xor(best, m);
        const int oa = __shfl_xor(best_a, m);
        if (oq > best || (oq == best && oa < best_a)) { best = oq; best_a = oa; }
    }
    if (lane == 0) {
        v_cur[st] = best;
        policy[st] = (float)(g.s_lo + (double)best_a * A.ds);
    }
}

struct DpPlayOut {
    PairStats stats;
    float *trace_a, *trace_r, *trace_k;
};

// the trilinear look-up of one stage's table at a float32 state: coordinates and blend in float64, rounded once
__device__ __forceinline__ float dp_policy_action(const DpArgs &A, const float *__restrict__ tab, float k, float z, float e) {
    const grl_solow_dp_grid &g = A.g;
    const DpCoord ck = dp_coord(log((double)k), A.lk_lo, A.dlk, g.nk);
    const DpCoord cz = dp_coord((double)z, -g.z_max, A.dz, g.nz);
    int j0 = 0, j1 = 0;
    double fe = 0.0;
    if (A.ne > 1) {                                          // the nodes are not uniform: find the bracket
        double lo = g.e_nodes[0], hi = g.e_nodes[1], top = g.e_nodes[0];
#pragma unroll
        for (int j = 1; j < DP_NQ; ++j) if (j < A.ne) top = g.e_nodes[j];
        const double ee = fmin(fmax((double)e, g.e_nodes[0]), top);
#pragma unroll
        for (int j = 1; j < DP_NQ - 1; ++j)
            if (j < A.ne - 1 && g.e_nodes[j] <= ee) { j0 = j; lo = g.e_nodes[j]; hi = g.e_nodes[j + 1]; }
        j1 = j0 + 1;
        fe = (ee - lo) / (hi - lo);
    }
    const double b0 = dp_bilinear(tab, g.nz, A.ne, ck, cz, j0), b1 = dp_bilinear(tab, g.nz, A.ne, ck, cz, j1);
    return (float)((1.0 - fe) * b0 + fe * b1);
}

__global__ __launch_bounds__(64) void solow_dp_play_kernel(SolowParams S, SolowShockCoef C, DpArgs A, const float *__restrict__ policy,
                                                            int horizon, int max_steps, int trace_steps, DpPlayOut O) {
    const int env = blockIdx.x * 64 + threadIdx.x;          // a wave per workgroup: the waves spread over the CUs
    if (env >= S.E) return;
    const size_t E = S.E;
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
        const float s = dp_policy_action(A, policy + (size_t)stage * A.n_states, k, zr[7], er[7]);
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

// the checks grl_solow_dp_solve and grl_solow_dp_set_policy share; fills A
static int dp_prepare(grl_handle *h, const char *fn, const grl_solow_dp_grid *grid, int32_t horizon, DpArgs &A) {
    const std::string f(fn);
    if (h->cfg.env_kind != GRL_ENV_SOLOW) return fail(h, GRL_E_INVALID, f + ": not a Solow handle");
    if (h->cfg.solow_p != 1 || h->cfg.solow_q > 1)
        return fail(h, GRL_E_INVALID, f + ": the handle has p = " + std::to_string(h->cfg.solow_p) + ", q = " + std::to_string(h->cfg.solow_q) +
                                          "; the grid covers p = 1 and q in {0, 1} (the state grows by one dimension per lag)");
    if (!grid) return fail(h, GRL_E_INVALID, f + ": null argument");
    if (h->step_in_flight) return fail(h, GRL_E_INVALID, f + ": a step is in flight (grl_wait first)");
    const grl_solow_dp_grid &g = *grid;
    const int32_t lim = 1 << 20;
    if (g.nk < 2 || g.nz < 2 || g.ns < 2 || g.nk > lim || g.nz > lim || g.ns > 65536)
        return fail(h, GRL_E_INVALID, f + ": nk, nz and ns must be at least 2 (nk, nz <= 2^20, ns <= 65536)");
    if (g.nq < 1 || g.nq > DP_NQ) return fail(h, GRL_E_INVALID, f + ": nq must be in 1..15");
    if (horizon < 1) return fail(h, GRL_E_INVALID, f + ": horizon must be at least 1");
    if (!(g.k_lo > 0.0) || !(g.k_hi > g.k_lo) || !std::isfinite(g.k_hi)) return fail(h, GRL_E_INVALID, f + ": needs 0 < k_lo < k_hi");
    if (!(g.z_max > 0.0) || !std::isfinite(g.z_max)) return fail(h, GRL_E_INVALID, f + ": needs z_max > 0");
    if (!(g.s_lo >= 0.0) || !(g.s_hi > g.s_lo) || !(g.s_hi <= 1.0)) return fail(h, GRL_E_INVALID, f + ": needs 0 <= s_lo < s_hi <= 1");
    for (int j = 0; j < g.nq; ++j) {
        if (!std::isfinite(g.e_nodes[j]) || !std::isfinite(g.e_weights[j]) || (j > 0 && !(g.e_nodes[j] > g.e_nodes[j - 1])))
            return fail(h, GRL_E_INVALID, f + ": e_nodes must be finite and ascending, e_weights finite");
    }
    A = DpArgs{};
    A.g = g;
    for (int j = g.nq; j < DP_NQ; ++j) { A.g.e_nodes[j] = 0.0; A.g.e_weights[j] = 0.0; }
    A.ne = h->cfg.solow_q > 0 ? g.nq : 1;
    const size_t n_states = (size_t)g.nk * g.nz * A.ne;
    if (n_states > GRL_SOLOW_DP_MAX_TABLE_BYTES / 4 / (size_t)horizon)
        return fail(h, GRL_E_SIZE, f + ": the policy table (horizon * nk * nz * ne float32) would exceed " +
                                       std::to_string(GRL_SOLOW_DP_MAX_TABLE_BYTES) + " bytes");
    A.n_states = (int)n_states;
    A.lk_lo = log(g.k_lo);
    A.dlk = (log(g.k_hi) - A.lk_lo) / (double)(g.nk - 1);
    A.dz = (g.z_max + g.z_max) / (double)(g.nz - 1);
    A.ds = (g.s_hi - g.s_lo) / (double)(g.ns - 1);
    A.rho = (double)h->so.rho_z[0];
    A.theta = h->cfg.solow_q > 0 ? (double)h->so.rho_e[0] : 0.0;
    A.delta = h->cfg.solow_delta;
    return GRL_OK;
}

static int dp_grow_tables(grl_handle *h, size_t n_states, size_t table) {
    SolowDpState &d = h->sdp;
    const int rc = episode_reserve(h, d.cap_states, n_states, {buf(d.v[0]), buf(d.v[1])});
    return rc ? rc : episode_reserve(h, d.cap_table, table, {buf(d.policy)});
}

static void dp_keep(grl_handle *h, const DpArgs &A, int horizon, bool has_value) {
    SolowDpState &d = h->sdp;
    d.grid = A.g; d.rho = A.rho; d.theta = A.theta; d.ne = A.ne; d.horizon = horizon; d.has_value = has_value;
}

// DpArgs of the table the handle keeps
static DpArgs dp_kept(grl_handle *h) {
    const SolowDpState &d = h->sdp;
    const grl_solow_dp_grid &g = d.grid;
    DpArgs A{};
    A.g = g; A.ne = d.ne; A.n_states = g.nk * g.nz * d.ne;
    A.lk_lo = log(g.k_lo);
    A.dlk = (log(g.k_hi) - A.lk_lo) / (double)(g.nk - 1);
    A.dz = (g.z_max + g.z_max) / (double)(g.nz - 1);
    A.ds = (g.s_hi - g.s_lo) / (double)(g.ns - 1);
    A.rho = d.rho; A.theta = d.theta; A.delta = h->cfg.solow_delta;
    return A;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_solow_dp_solve(grl_handle *h, const grl_solow_dp_grid *grid, int32_t horizon) {
    if (!h) return GRL_E_INVALID;
    DpArgs A;
    int rc = dp_prepare(h, "grl_solow_dp_solve", grid, horizon, A);
    if (rc) return rc;
    hipSetDevice(h->cfg.device_id);
    SolowDpState &d = h->sdp;
    d.horizon = 0;
    if ((rc = dp_grow_tables(h, A.n_states, (size_t)horizon * A.n_states))) return rc;
    const dim3 grid_dim((A.n_states + 3) / 4), block(256);
    rc = episode_launch(h, [&] {
        for (int t = horizon - 1; t >= 0; --t)
            hipLaunchKernelGGL(solow_dp_stage_kernel, grid_dim, block, 0, h->stream, A, d.v[(t + 1) & 1], d.v[t & 1],
                               d.policy + (size_t)t * A.n_states, t == horizon - 1 ? 1 : 0);
    });
    if (rc) return rc;
    dp_keep(h, A, horizon, true);
    return GRL_OK;
}

int grl_solow_dp_set_policy(grl_handle *h, const grl_solow_dp_grid *grid, int32_t horizon, const float *policy_host) {
    if (!h) return GRL_E_INVALID;
    DpArgs A;
    int rc = dp_prepare(h, "grl_solow_dp_set_policy", grid, horizon, A);
    if (rc) return rc;
    if (!policy_host) return fail(h, GRL_E_INVALID, "grl_solow_dp_set_policy: null argument");
    hipSetDevice(h->cfg.device_id);
    SolowDpState &d = h->sdp;
    d.horizon = 0;
    const size_t table = (size_t)horizon * A.n_states;
    if ((rc = dp_grow_tables(h, A.n_states, table))) return rc;
    GRL_HIP(h, hipMemcpyAsync(d.policy, policy_host, table * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));              // the caller's array may go away
    dp_keep(h, A, horizon, false);
    return GRL_OK;
}

int grl_solow_dp_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowDpState &d = h->sdp;
    const size_t n_states = (size_t)d.grid.nk * d.grid.nz * d.ne;
    const EpisodeOut outs[] = {
        {"policy", d.policy, (size_t)d.horizon * n_states * 4},
        {"value", d.v[0], n_states * 8, d.has_value ? nullptr : "the table was set, not solved: it has no value function"}};
    return episode_read(h, "grl_solow_dp_read", GRL_ENV_SOLOW, "Solow", d.horizon != 0, "grl_solow_dp_solve or grl_solow_dp_set_policy", outs, nullptr,
                        which, host, bytes);
}

int grl_solow_dp_play(grl_handle *h, int32_t max_steps, int32_t trace_steps) {
    const char *fn = "grl_solow_dp_play";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SOLOW, "Solow", true)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    if (trace_steps < 0 || trace_steps > max_steps) return fail(h, GRL_E_INVALID, "grl_solow_dp_play: trace_steps must be in 0..max_steps");
    if ((rc = episode_check_idle(h, fn))) return rc;
    SolowDpState &d = h->sdp;
    if (d.horizon == 0) return fail(h, GRL_E_STATE, "grl_solow_dp_play: call grl_solow_dp_solve or grl_solow_dp_set_policy first");
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
    const DpArgs A = dp_kept(h);
    DpPlayOut O{};
    O.stats = d.stats; O.trace_a = d.trace_a; O.trace_r = d.trace_r; O.trace_k = d.trace_k;
    rc = episode_launch(h, [&] {
        hipLaunchKernelGGL(solow_dp_play_kernel, dim3((h->E + 63) / 64), dim3(64), 0, h->stream, S, C, A, d.policy, d.horizon, max_steps, trace_steps, O);
    });
    if (rc) return rc;
    d.played = h->E; d.trace_steps = trace_steps;
    return GRL_OK;
}

int grl_solow_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowDpState &d = h->sdp;
    const size_t envs = h->E, trace = (size_t)d.trace_steps * envs;
    const char *untraced = d.trace_steps == 0 ? "the last play kept no trace (trace_steps was 0)" : nullptr;
    const EpisodeOut outs[] = {
        {"actions", d.trace_a, trace * 4, untraced}, {"rewards", d.trace_r, trace * 4, untraced}, {"k", d.trace_k, trace * 4, untraced}};
    return episode_read(h, "grl_solow_dp_play_read", GRL_ENV_SOLOW, "Solow", d.played != 0, "grl_solow_dp_play", outs, d.err, which, host, bytes, &d.stats, envs);
}

}  // extern "C"
