/* goldsrl_neteval.h -- ConvSingleAgentPolicyNetwork evaluated on its Swarm handle, whole episodes without a host round trip (brought
 * in by goldsrl_net.h).
 *
 * Replaces the per-step host loop of the reference's eval monitor (fed_gym/agents/paac/policy_monitor.py:127-208: per step a
 * blocking predict, a numpy draw, transform_actions, env.step and four reads).  Every env of the handle plays one episode from
 * its CURRENT state, at most max_steps steps.  The net's forward is 6 MB of weights on the matrix pipe, so an episode is not one
 * kernel: it is the training rollout's pipeline -- per step and chunk of envs the forward pass, an action kernel, the env step with
 * its auto-reset and an accounting kernel, dealt to the lanes' streams as grl_net_rollout deals them -- with nothing read back
 * until the episodes are over.
 *
 * What is written: the handle's env state advances, as the host loop's does (x, xa, the observation, reward / done, elapsed and
 * episode counters, the done list); an env whose episode ended inside the call goes on being stepped from its auto-reset state,
 * and nothing of that is recorded.  The episode bookkeeping of grl_episodes_* is not run.  What is left exactly as it was: the
 * parameters, the optimizer state, the action counter, the resident activations with their version, and every buffer of the last
 * rollout (grl_net_read_rollout, grl_net_train_rollout still speak of it).
 */
#ifndef GOLDSRL_NETEVAL_H
#define GOLDSRL_NETEVAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* greedy != 0: the raw action is mu.  greedy == 0: mu + sigma * z in float64, rounded to float32, where z is normals_host[env][t]
 * [agent][0..1] when normals_host is given -- (E, max_steps, 10, 2) float64, copied before the call returns -- and otherwise the
 * rollout's keyed draw, block (seed, env + env_id_offset, action counter + t, stream 16, agent), the counter staying where it
 * is.  Either way the float32 norm clip follows and the env steps with the float32 row, as the rollout and the host loop's
 * float32 actions do.  keep_actions != 0 keeps every env's env actions, trace_env >= 0 the per-step heads of that env.
 * Asynchronous: enqueues on the handle's streams and marks a step in flight, as grl_net_rollout does; grl_wait(h) joins and clears
 * the mark (grl_net_read_eval drains the streams too, and leaves the mark alone).  Besides the join, a read must follow
 * every evaluation before the net's next gradient step: the range verdict of a rollout made before the evaluation (the word
 * grl_net_train_rollout asks) is set aside while the evaluation runs and put back by its first read (or by the next grl_net_eval).
 * GRL_E_INVALID: null net, max_steps outside 1..1024, a net of num_actions != 2, trace_env outside [-1, E), normals_host together
 * with greedy, a step in flight, an output of more than 2^31 - 1 elements. */
int grl_net_eval(grl_net *net, int32_t max_steps, int32_t greedy, const double *normals_host, int32_t keep_actions, int32_t trace_env);
/* which (E envs, S = max_steps): "rewards" (E,S) float64, zero past the length; "length" (E) int32; "finished" (E) uint8, 1 when
 * the env reported done inside the call; "actions" (E,S,10,2) float32, the env actions, zero past the length (keep_actions only);
 * of the traced env: "trace_mu" "trace_sigma" "trace_raw" (S,10,2) float32 and "trace_value" (S,10) float32.  Synchronises.
 * The first read after an evaluation asks whether one of its forward passes left the fp16 range (goldsrl_net.h, Arithmetic): then
 * the net moves to the fp32 form, the evaluation's outputs are invalid and the read returns GRL_E_RANGE -- reset the env and
 * evaluate again; with GRL_NET_RANGE_FALLBACK=off the net stays and the read fails alike.
 * GRL_E_STATE before the first evaluation (or after an invalid one) and for an output the last one did not keep, GRL_E_SIZE on a
 * wrong byte count, GRL_E_INVALID on an unknown name. */
int grl_net_read_eval(grl_net *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_NETEVAL_H */
