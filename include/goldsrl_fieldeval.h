/* goldsrl_fieldeval.h -- ConvPolicyVFieldNetwork evaluated on its Swarm handle, whole episodes in one launch (brought in by
 * goldsrl_fieldnet.h).
 *
 * Replaces the per-step host loop of an evaluation monitor (the reference never built one for this net; the loop it would run is
 * fed_gym/agents/paac/policy_monitor.py:127-208): every env of the handle plays one episode from its CURRENT state -- the
 * compact observation from the positions, the net's forward, the action, the env step -- inside one kernel, one workgroup per env.
 * The net must be bound to its handle (grl_fieldnet_rollout_bind).  The handle and the net are read only: env state, observation
 * outputs, episode records, generator counters, parameters, optimizer state, the action counter and the last rollout's buffers
 * are left as they were.  An episode ends after the step whose reward is >= 0 or that reaches the handle's TimeLimit
 * (max_episode_steps - elapsed, at least 1) -- finished = 1 -- or after max_steps; there is no auto-reset.
 */
#ifndef GOLDSRL_FIELDEVAL_H
#define GOLDSRL_FIELDEVAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* greedy != 0: the raw action is mu; else mu + sigma N(0,1) with the rollout's noise key, block (seed, env + env_id_offset,
 * action counter + t, stream 16, agent), the counter staying where it is.  Either way the float32 norm clip follows.
 * rows32 == 0: the clipped action is widened and the env steps with a float64 row (SwarmEnv.step called directly);
 * rows32 != 0: the env steps with the float32 row, as the training rollout does.  keep_actions != 0 keeps every env's actions,
 * trace_env >= 0 the per-step trace of that env.  Asynchronous on the handle's stream.  GRL_E_INVALID: null or unbound net,
 * max_steps < 1, trace_env outside [-1, E), a step in flight, an output of more than 2^31 - 1 elements.  GRL_E_STATE: an env of this
 * geometry does not fit 64 KB of LDS. */
int grl_fieldnet_eval(grl_fieldnet *net, int32_t max_steps, int32_t greedy, int32_t rows32, int32_t keep_actions, int32_t trace_env);
/* which (E envs, S = max_steps): "rewards" (E,S) float64, zero past the length; "length" (E) int32; "finished" (E) uint8;
 * "actions" (E,S,10,2) float64, the env actions (keep_actions only); of the traced env: "trace_mu" "trace_sigma" "trace_raw"
 * (S,10,2) "trace_value" (S) float32, "trace_locust_bins" (S,80,2) "trace_agent_bins" "trace_positions" (S,10,2) uint8 -- the
 * observation each step acted on -- and "trace_x" (S,80,2) "trace_xa" (S,10,2) float64, the positions after each step.
 * Synchronises.  GRL_E_STATE before the first evaluation or for an output the last one did not keep, GRL_E_SIZE on a wrong
 * byte count, GRL_E_INVALID on an unknown name. */
int grl_fieldnet_read_eval(grl_fieldnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_FIELDEVAL_H */
