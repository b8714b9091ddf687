/* goldsrl_gausseval.h -- greedy acting and greedy evaluation of the A3C Gaussian agent (goldsrl_gaussnet.h includes this header;
 * the net, its sizes and its conventions are described there).
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/worker.py:180-230         run_n_steps(stochastic=False) / get_greedy_action
 *   fed_gym/agents/a3c/policy_monitor.py:42-96   PolicyMonitor.eval_once, for every env of the handle at once
 *
 * grl_anet_eval is ONE kernel launch: a workgroup of 4 waves keeps 64 envs for the whole episode and runs per step the trunk, the
 * mu tower (the sigma and value towers are not evaluated), the greedy action, the env step, the window rule and the float64 reward
 * sum.  These are the device functions the per-step path (grl_anet_rollout with greedy on) runs, so the two agree bit for bit up
 * to each env's first done.  The evaluation feeds no episode records (grl_episodes_*).
 *
 * Why a header of its own: goldsrl_gaussnet.h is pinned by tests/test_oracle_gauss.py to the 17 functions of the training API
 * (declared = exported = bound in _ffi_gauss.ANET_SIGNATURES).  The three functions here are held to the same rule by
 * tests/test_gauss_eval_header.py against _ffi_gauss.ANET_EVAL_SIGNATURES.  A caller includes goldsrl_gaussnet.h and has both.
 */
#ifndef GOLDSRL_GAUSSEVAL_H
#define GOLDSRL_GAUSSEVAL_H

#include "goldsrl_gaussnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: grl_anet_rollout acts greedily -- raw = mu, "raw" reads back equal to "mu", nothing is drawn and the action counter
 * does not advance; windows, records, bootstrap, GAE and grl_anet_train_rollout as ever.  The default is 0. */
int grl_anet_set_greedy(grl_anet *net, int32_t on);
/* Greedy episodes of every env of the handle, from the handle's CURRENT state (the caller resets first, as eval_once does).
 * Every env's window restarts at its current observation (history = [state], policy_monitor.py:63-65) and follows the rollout's
 * window rule.  Action = sigmoid / tanh of mu.  An env stops at its first done; the call ends when every env has stopped or after
 * max_steps steps (max_steps >= 1, GRL_E_INVALID otherwise; trace_steps >= 0, capped at max_steps).  Async on the handle's
 * stream.  Afterwards the whole handle is reset as by grl_reset (for Solow with the tape draw), and the next rollout starts every
 * env's window anew.  Parameters, optimizer state, the action counter, the last rollout's buffers and the handle's episode
 * records are untouched. */
int grl_anet_eval(grl_anet *net, int32_t max_steps, int32_t trace_steps);
/* "total_reward" (E) float64: the float32 step rewards added in step order in float64 (total_reward += reward)
 * "length" (E) int32; "finished" (E) uint8: 0 where max_steps cut the episode
 * trace, the first S = min(trace_steps, steps played) steps (steps played = the longest episode), defined up to each env's own end:
 * "states" (S,E,S0) "mu" (S,E,A) "actions" (S,E,A) "rewards" (S,E) "dones" (S,E), float32.  Synchronises.
 * GRL_E_STATE before the first grl_anet_eval. */
int grl_anet_read_eval(grl_anet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_GAUSSEVAL_H */
