/* goldsrl_solowarmadp.h -- the optimal-savings yardstick of the Solow env for the orders goldsrl_solowdp.h refuses (Solow-2-2-*,
 * Solow-3-3-*, any p >= 1 with max(p, q + 1) <= 4): finite-horizon backward induction on the minimal state of the ARMA(p, q)
 * shock, one kernel launch per stage, and the play of the tabulated policy on every env of the handle, whole episodes in one
 * launch (csrc/solow_arma_dp.hip).
 *
 * Replaces nothing in the reference: fed_gym prints the constant-savings floor for (1,1), (2,2) and (3,3)
 * (scripts/constant_solow.py, here goldsrl_sweep.h) and nothing that says how much reward any of them holds.  This header is this
 * build's own, and stands beside goldsrl_solowdp.h, which it does not change.
 *
 * The model.  The env's state is (k, z lags, e lags), 1 + p + q numbers, but the savings rate never touches the shock, and an
 * ARMA(p, q) process is Markov in m = max(p, q + 1) numbers: the forecasts f_j = E_t[z_{t+j}], j = 0..m-1, f_0 = z_t.  With the
 * handle's rho_z, rho_e (float32, multiplying the lag arrays oldest first: fed_env.py:207-217) read as lag coefficients
 * phi_l = rho_z[p - l], th_l = rho_e[q - l], and the impulse responses psi_0 = 1, psi_j = th_j + sum_{l=1..min(j,p)} phi_l psi_{j-l}:
 *   f'_j = f_{j+1} + psi_j eps (j < m-1);   f'_{m-1} = sum_{l=1..p} phi_l f_{m-l} + psi_{m-1} eps       i.e.  f' = A f + b eps
 *   f = Mz zv + Me ev                       the map from the env's lag arrays (oldest first), from the same recursion
 * A handle created with q = 0 keeps one innovation and rho_e = [0.5], as the reference's env does from its first step on; the
 * model is the handle's, so it reports q = 1 there.  Everything is float64, derived on the host; the kernels take (A, b, Mz, Me)
 * as data and know nothing of p and q.
 *   y = exp(f_0) * k^0.33;  r = log((1 - s) * y + 1e-4);  k' = (1 - delta) * k + s * y
 * The objective is the undiscounted sum of r over the remaining steps, the unit of eval/total_reward.
 *
 * Grids: k has nk points uniform in log k on [k_lo, k_hi]; axis j of f has nx[j] points uniform on [-x_max[j], x_max[j]]; s has
 * ns points uniform on [s_lo, s_hi]; eps has the nq quadrature nodes e_nodes (in units of the shock) with weights e_weights.
 *   W(f; k) = sum_j w_j sum_corners wt * V_next[corner of A f + b e_nodes[j]][k]        (nodes outer, corners ascending inner)
 *   Q(k, f; s) = r + lerp(W(f; .), log k')
 * Coordinates are clamped to the grid's edges, the arg-max takes the lowest index on a tie, the last stage has V_next = 0.
 * Tables are row-major (nx[0], .., nx[m-1], nk), k fastest.
 *
 * Held to declared = exported = bound (goldsrl/_ffi_solowarmadp.py) by tests/test_solow_arma_dp_header.py.
 */
#ifndef GOLDSRL_SOLOWARMADP_H
#define GOLDSRL_SOLOWARMADP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_SOLOW_ARMA_DP_MAX_DIM 4
#define GRL_SOLOW_ARMA_DP_MAX_LAGS 8
#define GRL_SOLOW_ARMA_DP_MAX_NODES 15
/* the most k points: the expectation slab of a shock node (nk float64) lives in a workgroup's LDS */
#define GRL_SOLOW_ARMA_DP_MAX_NK 4096
/* the largest policy table (horizon * nx[0] * .. * nx[m-1] * nk float32) a handle keeps: 1 GiB */
#define GRL_SOLOW_ARMA_DP_MAX_TABLE_BYTES ((size_t)1 << 30)

typedef struct grl_solow_arma_coef {
    double A[GRL_SOLOW_ARMA_DP_MAX_DIM * GRL_SOLOW_ARMA_DP_MAX_DIM];      /* row-major (4, 4); rows and columns >= m are zero */
    double b[GRL_SOLOW_ARMA_DP_MAX_DIM];                                  /* psi_0 .. psi_{m-1} */
    double Mz[GRL_SOLOW_ARMA_DP_MAX_DIM * GRL_SOLOW_ARMA_DP_MAX_LAGS];    /* row-major (4, 8): Mz[j * 8 + i] multiplies zv[i], i < p */
    double Me[GRL_SOLOW_ARMA_DP_MAX_DIM * GRL_SOLOW_ARMA_DP_MAX_LAGS];    /* row-major (4, 8): Me[j * 8 + i] multiplies ev[i], i < q */
    double f_std[GRL_SOLOW_ARMA_DP_MAX_DIM];   /* stationary deviation of f_j: sigma * sqrt(sum_{i<1024} (A^i b)_j^2) */
    int32_t m, p, q;
} grl_solow_arma_coef;

typedef struct grl_solow_arma_dp_grid {
    double k_lo, k_hi;                                 /* 0 < k_lo < k_hi */
    double x_max[GRL_SOLOW_ARMA_DP_MAX_DIM];           /* > 0 for j < m */
    double s_lo, s_hi;                                 /* 0 <= s_lo < s_hi <= 1 */
    double e_nodes[GRL_SOLOW_ARMA_DP_MAX_NODES];       /* in units of the shock (sigma * x_j) */
    double e_weights[GRL_SOLOW_ARMA_DP_MAX_NODES];
    int32_t nk, ns, nq;                                /* 2 <= nk <= 4096, 2 <= ns <= 65536, 1 <= nq <= 15 */
    int32_t nx[GRL_SOLOW_ARMA_DP_MAX_DIM];             /* >= 2 for j < m; entries from m on are not read */
} grl_solow_arma_dp_grid;

/* The handle's model.  No device work.
 * GRL_E_INVALID: null handle or argument, not a Solow handle, p < 1 or m = max(p, q + 1) > 4 (the message names m). */
int grl_solow_arma_model(grl_handle *h, grl_solow_arma_coef *model);

/* Backward induction over horizon >= 1 stages; stage horizon-1 is the episode's last step.  One launch per stage on the handle's
 * stream, V double-buffered in float64.  Keeps every stage's policy (horizon, nx[0], .., nx[m-1], nk) float32 and stage 0's value
 * function in float64; both replace what an earlier solve or set_policy left.  The handle's env state is untouched.  Async.
 * GRL_E_INVALID: as grl_solow_arma_model, or a bad grid or horizon, a step in flight.
 * GRL_E_SIZE: the policy table would exceed GRL_SOLOW_ARMA_DP_MAX_TABLE_BYTES. */
int grl_solow_arma_dp_solve(grl_handle *h, const grl_solow_arma_dp_grid *grid, int32_t horizon);
/* Uploads policy_host (horizon, nx[0], .., nx[m-1], nk) float32 in place of a solved table; the nodes and weights of the grid are
 * not used.  There is no value function afterwards.  Errors as grl_solow_arma_dp_solve. */
int grl_solow_arma_dp_set_policy(grl_handle *h, const grl_solow_arma_dp_grid *grid, int32_t horizon, const float *policy_host);
/* "policy" (horizon, nx[0], .., nx[m-1], nk) f32; "value" (nx[0], .., nx[m-1], nk) f64, stage 0's.  Synchronises.
 * GRL_E_STATE before any solve or set_policy, and for "value" after set_policy; GRL_E_SIZE on a wrong byte count. */
int grl_solow_arma_dp_read(grl_handle *h, const char *which, void *host, size_t bytes);

/* Every env of the handle plays a whole episode from its CURRENT state under the table, one lane per env, in one launch.  With
 * `remaining` the steps left to the handle's TimeLimit the step uses stage max(0, horizon - remaining), stage 0 without a
 * TimeLimit; s is the (m+1)-linear look-up of that stage at f = Mz zv + Me ev of the env's float32 lags and at its float32 k,
 * coordinates and blend in float64, clamped to the grid, rounded once to float32.  The step arithmetic is that of grl_step.  No
 * auto-reset: an env stops after max_steps steps, at its TimeLimit (finished = 1) or when its shock tape is empty (an error, as in
 * the step path).  The handle's env state, outputs, episode records and generator counters are untouched.  trace_steps in
 * [0, max_steps]: the first trace_steps steps of every env are kept.  Async.
 * GRL_E_INVALID: null handle, not a Solow handle, bad argument, a step in flight.  GRL_E_STATE: no table yet. */
int grl_solow_arma_dp_play(grl_handle *h, int32_t max_steps, int32_t trace_steps);
/* "total" "sum_sq" (E) f64, the float32 step rewards added in step order; "min" "max" (E) f32; "length" (E) i32; "finished" (E)
 * u8; "actions" "rewards" "k" (trace_steps, E) f32, defined up to the env's length, zero after it (GRL_E_STATE with
 * trace_steps = 0).  Synchronises.  GRL_E_STATE before the first play, or when an env ran off its tape. */
int grl_solow_arma_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SOLOWARMADP_H */
