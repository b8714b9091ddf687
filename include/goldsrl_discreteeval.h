/* goldsrl_discreteeval.h -- greedy acting and greedy evaluation of the A3C discrete savings-grid agent (goldsrl_discretenet.h
 * includes this header; the net, its sizes and its conventions are described there).
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/worker.py:360-376         GridSolowWorker.get_action_from_policy(stochastic=False) / get_greedy_action
 *   fed_gym/agents/a3c/policy_monitor.py:42-96   PolicyMonitor.eval_once, for every env of the handle at once
 *
 * The greedy rule.  The reference's greedy path through run_n_steps cannot run: get_greedy_action returns the grid VALUE of the
 * arg-max, and run_n_steps hands that float to transform_raw_action, which indexes it (worker.py:370-376).  The device form takes
 * the evident intention, as scripts/train_trade.py does for TradeWorker: choice = the first index of the largest float32
 * probability (np.argmax), action = grid[choice].  Nothing is drawn and the action counter stands still.
 *
 * grl_dnet_eval is ONE kernel launch: a workgroup of 4 waves keeps 64 envs for the whole episode and runs per step the trunk, the
 * probs tower (the value tower is not evaluated), the softmax, the arg-max, the env step, the window rule and the float64 reward
 * sum.  These are the device functions the per-step path (grl_dnet_rollout with greedy on) runs, so the two agree bit for bit up
 * to each env's first done.  The evaluation feeds no episode records (grl_episodes_*).
 */
#ifndef GOLDSRL_DISCRETEEVAL_H
#define GOLDSRL_DISCRETEEVAL_H

#include "goldsrl_discretenet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: grl_dnet_rollout acts greedily -- "choices" is the arg-max of "probs" (first index on ties), nothing is drawn and the
 * action counter does not advance; windows, records, bootstrap, GAE and grl_dnet_train_rollout as ever.  The default is 0. */
int grl_dnet_set_greedy(grl_dnet *net, int32_t on);
/* Greedy episodes of every env of the handle, from the handle's CURRENT state (the caller resets first, as eval_once does).
 * Every env's window restarts at its current observation (history = [state], policy_monitor.py:63-65) and follows the rollout's
 * window rule.  An env stops at its first done; the call ends when every env has stopped or after max_steps steps (max_steps >= 1,
 * GRL_E_INVALID otherwise; trace_steps >= 0, capped at max_steps).  Async on the handle's stream.  Afterwards the whole handle is
 * reset as by grl_reset (with the tape draw), and the next rollout starts every env's window anew.  Parameters, optimizer state,
 * the action counter, the last rollout's buffers and the handle's episode records are untouched. */
int grl_dnet_eval(grl_dnet *net, int32_t max_steps, int32_t trace_steps);
/* "total_reward" (E) float64: the float32 step rewards added in step order in float64 (total_reward += reward)
 * "length" (E) int32; "finished" (E) uint8: 0 where max_steps cut the episode
 * trace, the first S = min(trace_steps, steps played) steps (steps played = the longest episode), defined up to each env's own end:
 * "states" (S,E,2) float32, "choices" (S,E) int32, "actions" (S,E) "rewards" (S,E) "dones" (S,E) float32.  Synchronises.
 * GRL_E_STATE before the first grl_dnet_eval. */
int grl_dnet_read_eval(grl_dnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_DISCRETEEVAL_H */
