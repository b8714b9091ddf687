/* goldsrl_swarmcemplan.h -- search planner on the Swarm env: at every decision each env tunes the five real numbers of a feedback
 * rule (cancel, gain, off_x, off_y, radius; the anchor is fixed) by a short cross-entropy search over lookaheads from where it
 * stands, compares the result with a library of rules, commits the better for `replan` steps and plans again; a whole planned
 * episode of every env enqueued in one call (csrc/swarm_cemplan.hip).  Nothing is read back between decisions or generations; the
 * handle is read only.
 *
 * It is grl_swarm_plan (goldsrl_swarmplan.h) with grl_swarm_search (goldsrl_swarmsearch.h) in the place of its table: the answer
 * to what a controller earns that reacts to the state and may pick ANY rule of the six-number family.  A rule is a row (cancel,
 * gain, anchor) and an offset table off[10][2] (goldsrl_swarmrules.h), its action the statements written there.  The env is
 * deterministic from a state (quirk Q1), so the lookahead plays the true model and knows nothing a policy could not.  The reference
 * has no counterpart.
 *
 * The scheme.  Everything is float64, one IEEE operation per statement (the library is built with -ffp-contract=off); max and min
 * are the search's: a >= b ? a : b and a <= b ? a : b, the first operand wins a tie.  k runs over (cancel, gain, off_x, off_y,
 * radius), d over the D = ceil(max_steps / replan) decisions, g over the G generations, c over the C candidates, r over the R
 * library rules.  Every env e runs the scheme on its own, with its own mean_e[5]; t is the number of steps it has committed and
 * elapsed = elapsed0 + t.
 *   1 start      at d = 0: mean_e[k] = min(max(mean0[k], lo[k]), hi[k]).  At every decision mean[d][0] = mean_e and
 *                std[d][0][k] = std0[k]: the spread is reset, only the mean is carried over.
 *   2 generation statements 2 to 4 of goldsrl_swarmsearch.h from mean[d][g], std[d][g] and the normals z[d][g][c], which all envs
 *                share: v = std * z; v = mean + v; v = max(v, lo); v = min(v, hi); rule row (cancel, gain, anchor); t = radius *
 *                ring[a][0]; off[a][0] = off_x + t; likewise [1].  Candidate 0 is the incumbent and its row of z is ignored: for g = 0
 *                the row of mean_e, afterwards a bit-for-bit copy of the best candidate of the generation before.
 *   3 evaluate   every candidate plays min(horizon, TimeLimit - elapsed) steps ahead from the env's working state, exactly
 *                grl_swarm_plan's lookahead: score s = 0.0; s = s + r_t in step order, ended by a reward >= 0 or the TimeLimit, not
 *                shortened by max_steps.  The R library rules are scored the same way, once per decision.
 *   4 refit      statements 7 and 8 of goldsrl_swarmsearch.h per env over the M elites; the fit of a candidate is the env's own score
 *                (the search with one env gives the same bits: 0.0 + s and s / 1.0 are s, a score is never zero).  mean[d][g + 1],
 *                std[d][g + 1].
 *   5 choose     best_lib: the first index of the largest library score (a strict > from index 0; none when R = 0).  The searched
 *                candidate is rank 0 of generation G - 1.  It is chosen if R = 0 or its score is strictly larger than the library's
 *                best, otherwise the library rule is: a tie goes to the library.  choices[e][d] is the library index, or R for
 *                "searched".
 *   6 commit     min(replan, max_steps - t) steps of the chosen rule from the working state, as grl_swarm_plan commits: each step
 *                the step of grl_swarm_step_f64 on the rule's action row, wind added.  If the choice was the searched rule, mean_e
 *                becomes its five numbers, bit for bit; otherwise mean_e stays.  The env ends after the step whose reward is >= 0
 *                or that reaches the TimeLimit (finished = 1), or after max_steps.  No auto-reset; an ended env takes part in nothing
 *                further, and every output row past its end is zero (choices: -1).
 * The device evaluates no transcendental function for the search: the normals and the ring come from the host.  The handle's Swarm
 * math mode selects the step's arithmetic only.  Per decision 2 G + 2 kernels on the handle's stream: per generation the lookahead
 * (the planner's kernel over a table per env; generation 0's launch also plays the library rows) and one workgroup per env for rank,
 * refit and the next rows, after the last generation also the choice; then the planner's commit.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_swarm_cemplan_header.py against
 * _ffi_swarmcemplan.SWARMCEMPLAN_SIGNATURES.
 */
#ifndef GOLDSRL_SWARMCEMPLAN_H
#define GOLDSRL_SWARMCEMPLAN_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rules_host: (n_rules, 3) float64 rows (cancel, gain, anchor); offsets_host: (n_rules, 10, 2) float64; 0 <= n_rules <= 4096, both
 * may be null when n_rules is 0.  anchor: 0 (the centroid) or 1 (the agent's nearest locust), the searched rules' anchor.  mean0,
 * std0, floor, lo, hi: 5 float64 each over (cancel, gain, off_x, off_y, radius).  ring: (10, 2) float64.  normals: (D, G, C, 5)
 * float64 with D = ceil(max_steps / replan).  1 <= replan <= horizon; G >= 1 generations, 2 <= C <= 1024 candidates, 1 <= M <= C
 * elites; max_steps >= 1; trace_env in [-1, E): the committed steps of that env are traced.  keep_actions != 0 keeps every
 * committed action row.  Plays every env from the handle's CURRENT state (the caller resets first) on a working copy of its own: the
 * handle's env state, outputs, episode records and generator counters are untouched.  Async on the handle's stream; the host arrays
 * may be reused on return.
 * GRL_E_INVALID: null handle or argument, not a Swarm handle, an anchor that is not 0 or 1, a number that is not finite, std0 < 0,
 * floor < 0, lo > hi, a bad n_rules, horizon, replan, G, C, M, max_steps or trace_env, a step in flight, an output of more than
 * 2^31 - 1 elements. */
int grl_swarm_cemplan(grl_handle *h, const double *rules_host, const double *offsets_host, int32_t n_rules, int32_t anchor,
                      const double *mean0, const double *std0, const double *floor, const double *lo, const double *hi, const double *ring,
                      const double *normals, int32_t horizon, int32_t replan, int32_t G, int32_t C, int32_t M, int32_t max_steps,
                      int32_t keep_actions, int32_t trace_env);
/* "rewards" (E,max_steps) f64; "length" (E) i32; "finished" (E) u8; "choices" (E,D) i32, -1 past the env's last decision;
 * "chosen_rules" (E,D,3) f64 and "chosen_offsets" (E,D,10,2) f64, the committed rule; "lib_scores" (E,D,n_rules) f64 (GRL_E_STATE when
 * n_rules was 0); "candidates" (E,D,G,C,6) f64, the six-number rows as played; "scores" (E,D,G,C) f64; "order" (E,D,G,C) i32; "mean"
 * (E,D,G+1,5) f64 and "std" (E,D,G+1,5) f64, row 0 the decision's start; "actions" (E,max_steps,10,2) f64 (GRL_E_STATE without
 * keep_actions); "trace_x" (max_steps,80,2) f64 and "trace_xa" (max_steps,10,2) f64: the positions after every committed step of the
 * traced env (GRL_E_STATE without trace_env).  Everything is zero past the env's end.  Totals are the host's.  Synchronises.
 * GRL_E_STATE before the first run, GRL_E_SIZE on a wrong byte count. */
int grl_swarm_cemplan_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SWARMCEMPLAN_H */
