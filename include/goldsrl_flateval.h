/* goldsrl_flateval.h -- greedy acting and whole-episode evaluation of the flat PAAC policy (goldsrl_flatnet.h includes this header;
 * the net, its sizes and its conventions are described there).
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/paac/policy_monitor.py:84-108   SolowPolicyMonitor.eval_once, for every env of the handle at once
 *   fed_gym/agents/paac/paac.py:63-77              the monitor PAACLearner.train starts beside the training loop
 * TradeAR1 under the flat net has no monitor in the reference; it is evaluated the same way.
 *
 * grl_fnet_eval is ONE kernel launch: a workgroup keeps 16 / 32 / 64 envs (the rule of the persistent rollout, GRL_FLAT_GROUP) for
 * the whole episode and runs per step the window length, the forward, the action, the env step and the float64 reward sum.  These
 * are the device functions grl_fnet_rollout runs, so the two agree bit for bit up to each env's first done.  Workgroups share
 * nothing: any number of envs is legal.  The evaluation feeds no episode records (grl_episodes_*).
 *
 * Window: the rollout's -- min(max(nhist, 1), rnn_length) copies of the current state, the window the policy is trained under.
 * The reference monitor feeds the true last rnn_length states; the host-driven SolowPolicyMonitor keeps that window.
 *
 * Why a header of its own: tests/test_cabi_symbols.py pins the text of goldsrl_flatnet.h to _ffi_flat.FNET_SIGNATURES.  The three
 * functions here are held to the same rule by tests/test_flat_eval_header.py against _ffi_flat.FNET_EVAL_SIGNATURES.  A caller
 * includes goldsrl_flatnet.h and has both.
 */
#ifndef GOLDSRL_FLATEVAL_H
#define GOLDSRL_FLATEVAL_H

#include "goldsrl_flatnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: grl_fnet_rollout acts with raw = mu (by selection, nothing is drawn) in both of its forms; "actions" reads back equal
 * to mu and the action counter does not advance; everything else as ever.  The default is 0. */
int grl_fnet_set_greedy(grl_fnet *net, int32_t on);
/* Episodes of every env of the handle, from the handle's CURRENT state (the caller resets first).  greedy == 0: raw = mu + sigma *
 * N(0,1) from the rollout's stream at counters action_counter + t, and the action counter advances by max_steps (as
 * grl_fnet_rollout(T) advances it by T); greedy != 0: raw = mu and the counter does not move.  An env stops at its first done; the
 * call ends when every env has stopped or after max_steps steps (max_steps >= 1 and trace_steps >= 0, GRL_E_INVALID otherwise;
 * trace_steps is capped at max_steps).  Async on the handle's stream.  Afterwards the whole handle is reset as by grl_reset (for
 * Solow with the tape draw).  Parameters, optimizer state, the last rollout's buffers, the training workspace, the handle's
 * episode records and the form the rollout takes are untouched.  GRL_E_STATE when the net holds none of the process's 64
 * constant-memory argument slots (more than 64 live flat nets; grl_fnet_rollout then runs as a graph of launches, the evaluation
 * has no such form), GRL_E_SIZE when the handle has more envs than the net's max_samples. */
int grl_fnet_eval(grl_fnet *net, int32_t max_steps, int32_t trace_steps, int32_t greedy);
/* "total_reward" (E) float64: the float32 step rewards added in step order in float64
 * "length" (E) int32; "finished" (E) uint8: 0 where max_steps cut the episode
 * trace, the first S = min(trace_steps, steps played) steps (steps played = the longest episode), defined up to each env's own end:
 * "states" (S,E,S0) float32, "nhist" (S,E) int32, "mu" "sigma" "raw" "actions" (the env's) (S,E,A) float32,
 * "values" "rewards" "dones" (S,E) float32.  Synchronises.  GRL_E_STATE before the first grl_fnet_eval, GRL_E_SIZE for a wrong
 * size. */
int grl_fnet_read_eval(grl_fnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_FLATEVAL_H */
