/* goldsrl_gatedeval.h -- greedy acting and greedy evaluation of the Ticker gated trader (goldsrl_gatednet.h includes this header;
 * the net, its sizes and its conventions are described there).
 *
 * The reference has no counterpart: TickerGatedTraderWorker.get_action_from_policy (fed_gym/agents/a3c/worker.py:466-476) ignores
 * its `stochastic` argument, and no PolicyMonitor is written for this worker.  The greedy rule is fixed here, per asset:
 *   choice   = the first index of the largest of the three float32 probabilities (np.argmax, as GridSolowWorker.get_greedy_action
 *              picks its grid point, worker.py:370-372; a tie goes to the lower index)
 *   raw      = mu[choice]
 *   fraction = (float)(1 / (1 + exp(-(double)raw))), the worker's own transform (worker.py:229-230, 491-494)
 *
 * grl_gnet_eval is ONE kernel launch: a workgroup of 4 waves keeps 64 envs for the whole episode and runs per step the trunk, the
 * class tower and its softmax, the normal tower for mu (the value tower is not evaluated), the greedy pick, the Ticker step, the
 * window rule and the float64 reward sum.  These are the device functions the per-step path (grl_gnet_rollout with greedy on) runs,
 * so the two agree bit for bit up to each env's first done.  The evaluation feeds no episode records (grl_episodes_*).
 *
 * Why a header of its own: goldsrl_gatednet.h is pinned by tests/test_oracle_gated.py to the 17 functions of the training API
 * (declared = exported = bound in _ffi_gated.GNET_SIGNATURES).  The three functions here are held to the same rule by
 * tests/test_gated_eval_header.py against _ffi_gated.GNET_EVAL_SIGNATURES.  A caller includes goldsrl_gatednet.h and has both.
 */
#ifndef GOLDSRL_GATEDEVAL_H
#define GOLDSRL_GATEDEVAL_H

#include "goldsrl_gatednet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: grl_gnet_rollout acts greedily by the rule above -- "raw" reads back equal to the chosen "mu", nothing is drawn and the
 * action counter does not advance; windows, records, bootstrap, GAE and grl_gnet_train_rollout as ever.  The default is 0. */
int grl_gnet_set_greedy(grl_gnet *net, int32_t on);
/* Greedy episodes of every env of the handle, from the handle's CURRENT state (the caller resets first).  Every env's window
 * restarts at its current observation and follows the rollout's window rule.  An env stops at its first done; the call ends when
 * every env has stopped or after max_steps steps (max_steps >= 1, GRL_E_INVALID otherwise; trace_steps >= 0, capped at max_steps).
 * GRL_E_STATE without a price table, and on a handle created with max_episode_steps = 0 (without a cap an env could step past row
 * 1023 of its price window).  Async on the handle's stream.  Afterwards the whole handle is reset as by grl_reset, and the next
 * rollout starts every env's window anew.  Parameters, optimizer state, the action counter, the last rollout's buffers and the
 * handle's episode records are untouched. */
int grl_gnet_eval(grl_gnet *net, int32_t max_steps, int32_t trace_steps);
/* "total_reward" (E) float64: the float32 step rewards added in step order in float64
 * "length" (E) int32; "finished" (E) uint8: 0 where max_steps cut the episode
 * trace, the first S = min(trace_steps, steps played) steps (steps played = the longest episode), defined up to each env's own end:
 * "states" (S,E,7) "probs" (S,E,2,3) "mu" (S,E,2,3) "actions" (S,E,4) "rewards" (S,E) "dones" (S,E) float32, "choices" (S,E,2) int32.
 * Synchronises.  GRL_E_STATE before the first grl_gnet_eval. */
int grl_gnet_read_eval(grl_gnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_GATEDEVAL_H */
