/* goldsrl_swarmplan.h -- receding-horizon rule planner on the Swarm env: look ahead, commit, replan, a whole planned episode of
 * every env enqueued in one call (csrc/swarm_plan.hip).
 *
 * The table is grl_swarm_rules' (goldsrl_swarmrules.h): rows (cancel, gain, anchor) and an offset table off[10][2] per rule, the
 * action of a rule the statements written there.  SwarmEnv.t stops at 10 after the burn-in (quirk Q1): every step reuses one
 * noise row, so from a given state the env is deterministic and a lookahead with the true model uses nothing a policy could not
 * know.  The reference has no counterpart.
 *
 * Per env, with t the number of steps committed and elapsed = elapsed0 + t:
 *   look ahead  every rule r plays min(horizon, TimeLimit - elapsed) steps from the env's working state, exactly as
 *               grl_swarm_rules(max_steps = horizon) would from that state; it ends after a reward >= 0 or at the TimeLimit.  max_steps
 *               does not shorten it.  score[r] is the float64 sum of those rewards in step order: s = 0.0; s = s + r_t.
 *   choose      the first index of the largest score (a strict > in index order from rule 0).
 *   commit      min(replan, max_steps - t) steps of the chosen rule from the working state, each step the step of
 *               grl_swarm_step_f64 on the rule's row, wind added.  The env ends after the step whose reward is >= 0 or that reaches
 *               the TimeLimit (finished = 1), or after max_steps.  No auto-reset; an ended env takes part in nothing further.
 * D = ceil(max_steps / replan) decisions, two kernels each, all on the handle's stream; nothing is read back between them.  The
 * handle's Swarm math mode selects the step's arithmetic only, never the rule's.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_swarm_plan_header.py against _ffi_swarmplan.SWARMPLAN_SIGNATURES.
 */
#ifndef GOLDSRL_SWARMPLAN_H
#define GOLDSRL_SWARMPLAN_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rules_host: (n_rules, 3) float64 rows (cancel, gain, anchor); offsets_host: (n_rules, 10, 2) float64.  1 <= n_rules <= 4096;
 * 1 <= replan <= horizon; max_steps >= 1; trace_env in [-1, E): the committed steps of that env are traced.  keep_actions != 0 keeps
 * every committed action row.  Plays every env from the handle's CURRENT state (the caller resets first) on a working copy of its
 * own: the handle's env state, outputs, episode records and generator counters are untouched.  Async on the handle's stream; the host
 * arrays may be reused on return.
 * GRL_E_INVALID: null handle or argument, not a Swarm handle, an anchor that is not 0 or 1, a rule number or offset that is not
 * finite, a bad argument, a step in flight, an output of more than 2^31 - 1 elements. */
int grl_swarm_plan(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t horizon, int32_t replan,
                   int32_t max_steps, int32_t keep_actions, int32_t trace_env);
/* With D = ceil(max_steps / replan): "rewards" (E,max_steps) f64, zero past the env's length; "length" (E) i32; "finished" (E) u8;
 * "choices" (E,D) i32, -1 past the env's last decision; "scores" (E,D,n_rules) f64, zero past it; "actions" (E,max_steps,10,2) f64,
 * zero past the length (GRL_E_STATE without keep_actions); "trace_x" (max_steps,80,2) f64 and "trace_xa" (max_steps,10,2) f64: the
 * positions after every committed step of the traced env, zero past the length (GRL_E_STATE without trace_env).  Totals are the
 * host's.  Synchronises.  GRL_E_STATE before the first run, GRL_E_SIZE on a wrong byte count. */
int grl_swarm_plan_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SWARMPLAN_H */
