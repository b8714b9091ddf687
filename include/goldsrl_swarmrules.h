/* goldsrl_swarmrules.h -- closed-loop feedback rules on the Swarm env: every (env, rule) pair plays a whole episode in one kernel
 * launch (csrc/swarm_rules.hip), the action of every step computed on the device from the positions the step before left.
 *
 * The reference has no counterpart: its only scripted play is scripts/make_swarm_gif.py:62-82, which replays recorded actions
 * (goldsrl_replay.h).  What a rule borrows from it is the clip of agents/paac/emulator_runner.py:113-118 in float64, so a rule
 * moves an agent no further than the policy can.
 *
 * A rule is (cancel, gain, anchor) and an offset table off[10][2].  Before each step agent a of a pair, in float64, one IEEE
 * operation per statement, on the positions as they stand before the step:
 *   anchor 0   cx = 0.0; for j in 0..79: cx = cx + x[j]; cx = cx / 80.0; likewise cy      (a sequential sum in index order)
 *   anchor 1   (cx, cy) = the locust with the smallest dx*dx + dy*dy, dx = x[j] - xa_x, dy = y[j] - xa_y   (strict <: the first wins)
 *   tx = cx + off[a][0];  ty = cy + off[a][1]
 *   ax = gain * (tx - xa_x) - cancel;  ay = gain * (ty - xa_y)
 *   d = sqrt(ax*ax + ay*ay);  if (d >= 1.0) { ax = ax / d; ay = ay / d; }
 * and the step is the step of grl_swarm_step_f64 on that row, wind added.  (0, 0, .) is the zero action, (1, 0, .) the action
 * (-1, 0) that cancels the wind.  The handle's Swarm math mode selects the step's arithmetic only, never the rule's.
 * There is no auto-reset: a pair ends after the step whose reward is >= 0 or that reaches the env's TimeLimit (finished = 1), or
 * after max_steps.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_swarm_rules_header.py against _ffi_swarmrules.SWARMRULES_SIGNATURES.
 */
#ifndef GOLDSRL_SWARMRULES_H
#define GOLDSRL_SWARMRULES_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rules_host: (n_rules, 3) float64 rows (cancel, gain, anchor); offsets_host: (n_rules, 10, 2) float64.  1 <= n_rules <= 4096;
 * max_steps >= 1; trace_env in [-1, E): all n_rules episodes of that env are traced.  keep_actions != 0 keeps every action row.
 * Plays every pair from the handle's CURRENT state (the caller resets first).  The handle's env state, outputs, episode records
 * and generator counters are untouched.  Async on the handle's stream; the host arrays may be reused on return.
 * GRL_E_INVALID: null handle or argument, not a Swarm handle, an anchor that is not 0 or 1, a rule number or offset that is not
 * finite, a bad argument, a step in flight, an output of more than 2^31 - 1 elements. */
int grl_swarm_rules(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t max_steps,
                    int32_t keep_actions, int32_t trace_env);
/* "rewards" (E,n_rules,max_steps) f64, zero past the pair's length; "length" (E,n_rules) i32; "finished" (E,n_rules) u8;
 * "actions" (E,n_rules,max_steps,10,2) f64, zero past the length (GRL_E_STATE without keep_actions); "trace_x"
 * (n_rules,max_steps,80,2) f64 and "trace_xa" (n_rules,max_steps,10,2) f64: the positions after every step of the traced env, zero
 * past the length (GRL_E_STATE without trace_env).  Totals are the host's.  Synchronises.  GRL_E_STATE before the first run,
 * GRL_E_SIZE on a wrong byte count. */
int grl_swarm_rules_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SWARMRULES_H */
