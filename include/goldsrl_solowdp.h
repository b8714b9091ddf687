/* goldsrl_solowdp.h -- the optimal-savings yardstick of the Solow env: finite-horizon backward induction on a grid, one kernel
 * launch per stage, and the play of the tabulated policy on every env of the handle, whole episodes in one launch
 * (csrc/solow_dp.hip).
 *
 * Replaces nothing in the reference: fed_gym has the constant-savings script (scripts/constant_solow.py, here goldsrl_sweep.h) and
 * nothing that says how much reward the model holds.  This header is this build's own.
 *
 * The model is the handle's, for p = 1 and q in {0, 1} (Solow-1-1-*, Solow-1-0-*, SolowSS-v0); every other order is refused,
 * because the state grows by one dimension per lag.  With rho = rho_z[0], theta = rho_e[0] (0 when q = 0), delta and sigma of the
 * handle and alpha = 0.33, all in float64:
 *   state (k, z, e), e the previous innovation; action s
 *   y = exp(z) * k^alpha;  r = log((1 - s) * y + 1e-4);  k' = (1 - delta) * k + s * y;  z' = (rho * z + theta * e) + eps;  e' = eps
 * The objective is the undiscounted sum of r over the remaining steps, the unit of eval/total_reward.
 *
 * Grids: k has nk points uniform in log k on [k_lo, k_hi]; z has nz points uniform on [-z_max, z_max]; e is exactly the nq
 * quadrature nodes e_nodes[j] = sigma * x_j (ascending) with weights e_weights[j] that sum to 1, so e' falls on a node and the
 * expectation needs no interpolation in e; with q = 0 the e-dimension has one point.  s has ns points uniform on [s_lo, s_hi].
 *   Q(k, z, e; s) = r + sum_j w_j * bilinear(V_next[:, :, j]; log k', (rho * z + theta * e) + e_nodes[j])
 * Coordinates are clamped to the grid's edges, the arg-max takes the lowest index on a tie, the last stage has V_next = 0.
 * Tables are row-major (nk, nz, ne), ne = nq for q = 1 and 1 for q = 0.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The functions here are held to the same rule by tests/test_solow_dp_header.py against _ffi_solowdp.SOLOW_DP_SIGNATURES.
 */
#ifndef GOLDSRL_SOLOWDP_H
#define GOLDSRL_SOLOWDP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_SOLOW_DP_MAX_NODES 15
/* the largest policy table (horizon * nk * nz * ne float32) a handle keeps: 1 GiB; the two float64 value buffers are
 * 2 / horizon of it.  The default grid (96 x 25 x 7, 256 stages) takes 17 MB. */
#define GRL_SOLOW_DP_MAX_TABLE_BYTES ((size_t)1 << 30)

typedef struct grl_solow_dp_grid {
    double k_lo, k_hi;                                 /* 0 < k_lo < k_hi */
    double z_max;                                      /* > 0 */
    double s_lo, s_hi;                                 /* 0 <= s_lo < s_hi <= 1 */
    double e_nodes[GRL_SOLOW_DP_MAX_NODES];            /* ascending, in units of the shock (sigma * x_j) */
    double e_weights[GRL_SOLOW_DP_MAX_NODES];
    int32_t nk, nz, nq, ns;                            /* nk, nz, ns >= 2 (ns <= 65536); 1 <= nq <= 15 */
} grl_solow_dp_grid;

/* Backward induction over horizon >= 1 stages; stage horizon-1 is the episode's last step.  One launch per stage on the handle's
 * stream, V double-buffered in float64.  Keeps every stage's policy (horizon, nk, nz, ne) float32 and stage 0's value function
 * in float64; both replace what an earlier solve or set_policy left.  The handle's env state is untouched.  Async.
 * GRL_E_INVALID: null handle, not a Solow handle, p != 1 or q > 1, a bad grid or horizon, a step in flight.
 * GRL_E_SIZE: the policy table would exceed GRL_SOLOW_DP_MAX_TABLE_BYTES. */
int grl_solow_dp_solve(grl_handle *h, const grl_solow_dp_grid *grid, int32_t horizon);
/* Uploads policy_host (horizon, nk, nz, ne) float32 in place of a solved table (a tabulated feedback rule from elsewhere); the
 * weights of the grid are not used.  There is no value function afterwards.  Errors as grl_solow_dp_solve. */
int grl_solow_dp_set_policy(grl_handle *h, const grl_solow_dp_grid *grid, int32_t horizon, const float *policy_host);
/* "policy" (horizon, nk, nz, ne) f32; "value" (nk, nz, ne) f64, stage 0's.  Synchronises.
 * GRL_E_STATE before any solve or set_policy, and for "value" after set_policy; GRL_E_SIZE on a wrong byte count. */
int grl_solow_dp_read(grl_handle *h, const char *which, void *host, size_t bytes);

/* Every env of the handle plays a whole episode from its CURRENT state under the table, one lane per env, in one launch.  With
 * `remaining` the steps left to the handle's TimeLimit the step uses stage max(0, horizon - remaining), stage 0 without a
 * TimeLimit; s is the trilinear look-up of that stage at the env's float32 (k, z, e), coordinates and blend in float64, clamped
 * to the grid, rounded once to float32.  The step arithmetic is that of grl_step.  No auto-reset: an env stops after max_steps
 * steps, at its TimeLimit (finished = 1) or when its shock tape is empty (an error, as in the step path).  The handle's env
 * state, outputs, episode records and generator counters are untouched.  trace_steps in [0, max_steps]: the first trace_steps
 * steps of every env are kept.  Async.
 * GRL_E_INVALID: null handle, not a Solow handle, bad argument, a step in flight.  GRL_E_STATE: no table yet. */
int grl_solow_dp_play(grl_handle *h, int32_t max_steps, int32_t trace_steps);
/* "total" "sum_sq" (E) f64, the float32 step rewards added in step order; "min" "max" (E) f32; "length" (E) i32; "finished" (E)
 * u8; "actions" "rewards" "k" (trace_steps, E) f32, defined up to the env's length, zero after it (GRL_E_STATE with
 * trace_steps = 0).  Synchronises.  GRL_E_STATE before the first play, or when an env ran off its tape. */
int grl_solow_dp_play_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SOLOWDP_H */
