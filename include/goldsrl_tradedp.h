/* goldsrl_tradedp.h -- the attainable optimum of the TradeAR1 env: finite-horizon backward induction over non-anticipating
 * policies on a (shares, log prices) grid, one kernel launch per stage, and the play of the tabulated policy on every env of the
 * handle, whole episodes in one launch (csrc/trade_dp.hip).
 *
 * Replaces nothing in the reference: fed_gym has no yardstick for TradeAR1.  grl_trade_foresight (goldsrl_tradeforesight.h) is the
 * trader who knows the coming prices; this is the best trader who does not, on the env's own stochastic model.  The played total
 * is attained by a feedback rule, so it is a lower bound on what can be learned; the foresight bound of the same path is above it.
 *
 * The model, float64, n = n_assets of the handle, which must be 1 or 2 (the grid grows by two dimensions per asset):
 *   W = cash + sum_a q_a p_a;  state: the value shares u_a = q_a p_a / W and the log prices x_a = log p_a;  c = 1 - sum_a u_a
 *   action a_a in [-1, 1], as TradeAR1Env._step moves the account, both branches on the cash the step began with:
 *     a_a > 0:  u'_a = u_a + (a_a / n) * c        otherwise:  u'_a = u_a * (1 + a_a)            c' = 1 - sum_a u'_a
 *   x'_a = 0.9 x_a + eps_a,  eps_a ~ N(0, std_e^2),  std_e^2 = std_p^2 (1 - 0.81);   R_a = exp(x'_a - x_a)
 *   g = c' + sum_a u'_a R_a;   u''_a = u'_a R_a / g
 * The step rewards telescope to log(W_last + 1e-4) - log(W_first + 1e-4); the model's objective is E sum log g.  It ignores the
 * 1e-4 and the `assets < 1` stop: both are outside a scale-free state.  The played episode has them, it runs the env's arithmetic.
 *
 * Recurrence: stage j has j price moves left; V_0 = 0;
 *   V_{j+1}(u, x) = max_a sum_k w_k [ log g + V_j(u'', x') ]
 * over the tensor product of nq quadrature nodes per asset, e_nodes[k] = std_e * x_k (ascending) with e_weights that sum to 1;
 * the joint nodes are walked with asset 0's index outermost and w_k = w_k0 * w_k1.  The look-up of V_j is 2n-linear with
 * coordinates clamped to the grid -- the price axes first (once per price node), then the share axes --, the arg-max takes the
 * lowest joint action index i_0 * na + i_1 on a tie.  One IEEE operation per statement, no contraction.
 *
 * Grids: u_a has nu points uniform on [0, 1]; for n = 2 a node with u_0 + u_1 > 1 stands for the state u / (u_0 + u_1), so every
 * node is a state.  x_a has nx points uniform on [-x_max, x_max].  Each action component has na points (2 i - (na - 1)) / (na - 1),
 * na odd so that 0 is a point.
 *
 * Tables, row-major: the policy (horizon, [nu]^n, [nx]^n, n) float32, row s the decisions with s + 1 moves left; the value
 * ([nu]^n, [nx]^n) float64 of the top stage, V_horizon.
 *
 * The functions here are held to declared = exported = bound in _ffi_tradedp.TRADE_DP_SIGNATURES by tests/test_trade_dp_header.py.
 */
#ifndef GOLDSRL_TRADEDP_H
#define GOLDSRL_TRADEDP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_TRADE_DP_MAX_NODES 15
/* the largest policy table (horizon * nu^n * nx^n * n float32) a handle keeps: 1 GiB, the cap of goldsrl_solowdp.h */
#define GRL_TRADE_DP_MAX_TABLE_BYTES ((size_t)1 << 30)
/* the LDS a workgroup of the solve can have: the slab of nq^n * nu^n float64 and 2 * n * nq + n * nq words beside it must fit */
#define GRL_TRADE_DP_MAX_LDS_BYTES ((size_t)160 * 1024)

typedef struct grl_trade_dp_grid {
    double x_max;                                      /* > 0 */
    double e_nodes[GRL_TRADE_DP_MAX_NODES];            /* ascending, in units of the shock (std_e * x_k) */
    double e_weights[GRL_TRADE_DP_MAX_NODES];
    int32_t nu, nx, na, nq;                            /* nu, nx >= 2; na >= 3 and odd; 1 <= nq <= 15 */
} grl_trade_dp_grid;

/* Backward induction over horizon >= 1 stages, one launch per stage on the handle's stream, V double-buffered in float64.  Keeps
 * the policy table and the top stage's value; both replace what an earlier solve or set_policy left.  The handle's env state is
 * untouched.  Async.
 * GRL_E_INVALID: null handle, not a TradeAR1 handle, n_assets above 2, a bad grid or horizon, a step in flight.
 * GRL_E_SIZE: the slab would exceed GRL_TRADE_DP_MAX_LDS_BYTES or the policy table GRL_TRADE_DP_MAX_TABLE_BYTES. */
int grl_trade_dp_solve(grl_handle *h, const grl_trade_dp_grid *grid, int32_t horizon);
/* Uploads policy_host (horizon, [nu]^n, [nx]^n, n) float32 in place of a solved table (a tabulated feedback rule from elsewhere);
 * na, nq, the nodes and the weights of the grid are not used beyond their checks.  There is no value afterwards.  Synchronises.
 * Errors as grl_trade_dp_solve, the slab's aside. */
int grl_trade_dp_set_policy(grl_handle *h, const grl_trade_dp_grid *grid, int32_t horizon, const float *policy_host);
/* "policy" (horizon, [nu]^n, [nx]^n, n) f32; "value" ([nu]^n, [nx]^n) f64.  Synchronises.
 * GRL_E_STATE before any solve or set_policy, and for "value" after set_policy; GRL_E_SIZE on a wrong byte count. */
int grl_trade_dp_read(grl_handle *h, const char *which, void *host, size_t bytes);

/* Every env of the handle plays a whole episode from its CURRENT state under the table, one lane per env, in one launch.  Per
 * step: u, x from the account in float64; with r the steps left to the handle's TimeLimit including this one, the moves left are
 * r - 1: row min(r - 1, horizon) - 1 of the table, the action 0 when r - 1 = 0, the top row without a TimeLimit; each action
 * component is the 2n-linear look-up of that row (price axes first, asset 1 innermost), clamped to the grid, rounded once to
 * float32; then the step arithmetic of grl_step.  normals_host: null (the handle's generator, at the counters its next steps would
 * use) or a tape (max_steps, n_assets, E) float32 whose row t moves the prices after step t, as grl_trade_sweep's.  No
 * auto-reset: an env stops after max_steps steps, at its TimeLimit (finished = 1) or when assets < 1 (finished = depleted = 1).
 * The handle is read only: state, generator counters, outputs, done list, episode records and the last results of the sweep,
 * foresight and search calls.  trace_steps in [0, max_steps]: the first trace_steps steps of every env are kept.  Async.
 * GRL_E_INVALID: null handle, not a TradeAR1 handle, bad argument, a handle with GRL_F_INJECT_NOISE and no tape, a step in
 * flight.  GRL_E_STATE: no table yet. */
int grl_trade_dp_play(grl_handle *h, const float *normals_host, int32_t max_steps, int32_t trace_steps);
/* "total" "sum_sq" "final_assets" (E) f64, the float32 step rewards added in step order; "min" "max" (E) f32; "length" (E) i32;
 * "finished" "depleted" (E) u8; "actions" (trace_steps, n_assets, E) f32, "rewards" (trace_steps, E) f32, "assets" (trace_steps,
 * E) f64 (after the step), defined up to the env's length, zero after it (GRL_E_STATE with trace_steps = 0).  Synchronises.
 * GRL_E_STATE before the first play. */
int grl_trade_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TRADEDP_H */
