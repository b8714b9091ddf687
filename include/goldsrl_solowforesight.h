/* goldsrl_solowforesight.h -- the perfect-foresight ceiling of the Solow env at ANY order (p, q): every env of the handle solves
 * its own episode by backward induction on capital alone, along the shock path its tape already fixes, and plays the plan, all in
 * one kernel launch (csrc/solow_foresight.hip).
 *
 * Replaces nothing in the reference: fed_gym prints the constant-savings floor (scripts/constant_solow.py, here goldsrl_sweep.h)
 * and nothing above it.  This header is this build's own and stands beside goldsrl_solowdp.h and goldsrl_solowarmadp.h, which it
 * does not change.
 *
 * Why it exists for every order.  SolowEnv._reset draws the whole innovation tape before the first step (fed_env.py:248), so the
 * path z_t of an episode is fixed at reset whatever the ARMA order; given the path the only state left is k.  The order is data:
 * the path is rolled forward with the step path's own float32 recursion, and a one-dimensional induction per env serves every
 * (p, q) a handle can hold -- the two induction solvers stop at m = max(p, q + 1) <= 4.
 *
 * Episode length.  For env e, L_e is the smallest of max_steps, the steps left to the handle's TimeLimit and the tape left.  An env
 * whose tape ends before the other two has its error counted, as in grl_solow_dp_play.
 *
 * The recurrence, all float64 and unfused; ez_t = (double)expf(z_t) is the per-step path's own float32 value, V_L = 0,
 * k_i = exp(log k_lo + i * dlk), s_a = s_lo + a * ds:
 *   y  = ez_t * k_i^0.33
 *   s' = max(1e-3, s_a)
 *   Q  = log((1 - s') * y + 1e-4) + lerp(V_{t+1}; log((1 - delta) * k_i + s' * y))      (coordinate clamped to the grid)
 *   V_t(k_i) = max_a Q, the lowest index on a tie; the decision is one byte per (env, t, i)
 * k_i^0.33 and (1 - delta) * k_i are computed once per node; delta is the handle's float64 solow_delta.
 *
 * The play starts from the env's current float32 k.  The rate of step t is the blend of the two bracketing nodes' rates
 * s_lo + a * ds in log k: coordinate and blend in float64, clamped to the grid, rounded once to float32 (the rule of the
 * inductions' plays in one dimension).  The step arithmetic is that of grl_step.
 *
 * What the figure is.  The played total is attained by a plan that knows the path, on a grid: it lies below the true ceiling.
 * V_0(k_0) is the grid's own value; on the paths measured here it lies above the played total and comes down to it as the grid
 * grows, so the two bracket the true ceiling there.  That is an observation, not a theorem.
 *
 * Held to declared = exported = bound (goldsrl/_ffi_solowforesight.py) by tests/test_solow_foresight_header.py.
 */
#ifndef GOLDSRL_SOLOWFORESIGHT_H
#define GOLDSRL_SOLOWFORESIGHT_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most k points (V double-buffered, two node tables and the decision rows live in a workgroup's LDS) and the most rates (a
 * decision is one byte) */
#define GRL_SOLOW_FORESIGHT_MAX_NK 1024
#define GRL_SOLOW_FORESIGHT_MAX_NS 256
/* the largest decision table (envs * max_steps * nk bytes) a launch fills: 1 GiB.  Envs beyond what fits are served by further
 * launches of the same kernel over the same table; GRL_SOLOW_FORESIGHT_TABLE_BYTES in the environment, read at the call, lowers
 * the cap. */
#define GRL_SOLOW_FORESIGHT_MAX_TABLE_BYTES ((size_t)1 << 30)

typedef struct grl_solow_foresight_grid {
    double k_lo, k_hi, s_lo, s_hi;      /* 0 < k_lo < k_hi, uniform in log k; 0 <= s_lo < s_hi <= 1, uniform */
    int32_t nk, ns;                     /* 2 <= nk <= 1024, 2 <= ns <= 256 */
} grl_solow_foresight_grid;

/* Every env of the handle, from its CURRENT state: the path, the induction over its L_e steps and the play, one workgroup per env,
 * in one launch (several when the decision table is capped).  No auto-reset.  The handle's env state, outputs, episode records and
 * generator counters are read only.  trace_steps in [0, max_steps]: the first trace_steps steps of every env are kept.  Async.
 * GRL_E_INVALID: null handle or grid, not a Solow handle, a bad grid, max_steps < 1, trace_steps outside 0..max_steps, a step in
 * flight.  GRL_E_SIZE: one env's table (max_steps * nk bytes) exceeds the cap.  The order is never refused. */
int grl_solow_foresight(grl_handle *h, const grl_solow_foresight_grid *grid, int32_t max_steps, int32_t trace_steps);
/* With T = max_steps of the last call:
 * "total" "sum_sq" (E) f64, the float32 step rewards added in step order; "min" "max" (E) f32; "length" (E) i32; "finished" (E) u8;
 * "value" (E) f64, V_0 interpolated at the env's k_0; "clamped" (E) i32, played steps whose k lay outside [k_lo, k_hi];
 * "ez" (T, E) f32, the path the induction saw, zero past L_e; "decisions" (E, T, nk) u8, zero past L_e (GRL_E_STATE when the call
 * took several launches); "actions" "rewards" "k" (trace_steps, E) f32, k after the step, zero past the length (GRL_E_STATE with
 * trace_steps = 0).  Synchronises.  GRL_E_STATE before the first call, or when an env ran off its tape. */
int grl_solow_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SOLOWFORESIGHT_H */
