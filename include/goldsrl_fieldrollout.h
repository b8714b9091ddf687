/* goldsrl_fieldrollout.h -- ConvPolicyVFieldNetwork acting and learning on a Swarm handle (brought in by goldsrl_fieldnet.h).
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/paac/paac.py:216-419              GridPAACLearner's loop body with the agent_positions feeds (:292,317,356,369,377)
 *   fed_gym/agents/state_processors.py:15-44         SwarmStateProcessor.process_state: the (grid, grid, 2) density image + .positions
 *   fed_gym/agents/paac/emulator_runner.py:113-118   SwarmRunner.transform_actions_for_env (norm clip)
 *
 * The net must sit on a Swarm handle with grid_size == height == width, channels == 2 and num_actions == 2; every call below
 * refuses anything else with GRL_E_INVALID before it launches.  Inputs of env e: state[bx][by][0] = (locusts of e in bin (bx, by))
 * / 80, state[bx][by][1] = (agents in that bin) / 10 as float32(count / 80.0), float32(count / 10.0); bins 255 are not counted;
 * the position of agent a is (positions[e][a][0], positions[e][a][1]).  The ten agents of an env share one image, so the trunk
 * (convs, dense stack, pol2, value tower) runs once per env and an agent reads its 2A columns of the mu / sigma fields.
 * B = 10 * E agent-samples in env-major order.  All sums run in a fixed order (no float atomics): bitwise reproducible.
 *
 * GRL_FIELD_FUSED=off in the environment (read at the net's first rollout call) runs the forward layer by layer on E env-samples
 * (chunked by max_samples) instead of one workgroup per env; a geometry whose env does not fit 64 KB of LDS takes that path anyway.
 * GRL_FIELD_HEADT=off reads the head columns from the stored row-major mu_w / sigma_w instead of the column-major copies.
 */
#ifndef GOLDSRL_FIELDROLLOUT_H
#define GOLDSRL_FIELDROLLOUT_H

#ifdef __cplusplus
extern "C" {
#endif

/* the discount of the n-step returns (the config struct has no slot for it); checks the geometry against the handle */
int grl_fieldnet_rollout_bind(grl_fieldnet *net, float gamma);
/* predict on the handle's CURRENT observation: mu (B,2) sigma (B,2) vs (B,) on the host (any may be NULL).  Synchronous. */
int grl_fieldnet_predict_swarm(grl_fieldnet *net, float *mu_host, float *sigma_host, float *vs_host);
/* the (n_envs, G, G, 2) float32 images the device builds from HOST observations (locust_bins (n,80,2), agent_bins (n,10,2) uint8) */
int grl_fieldnet_debug_grid(grl_fieldnet *net, int32_t n_envs, const uint8_t *locust_bins, const uint8_t *agent_bins, float *states_host,
                         size_t bytes);
/* T x (forward, a = mu + sigma N(0,1), norm clip, record the compact observation, env step, bookkeeping, reward layout 0 = per
 * agent-sample / 1 = the reference's first E columns), bootstrap forward, n-step returns.  Asynchronous (grl_wait); the action
 * counter advances by T.  Noise of (env, agent) at step t: block (seed, env + env_id_offset, counter + t, stream 16, agent). */
int grl_fieldnet_rollout(grl_fieldnet *net, int32_t T, int32_t reward_layout);
/* The reference loss (policy_v_network.py:154-173) as a mean over the T*B agent-samples of the last rollout, backward,
 * clip_by_global_norm, Adam(lr).  stats_host: {loss, policy_loss, critic_loss_mean, global_norm}.  _grads: stops before the clip. */
int grl_fieldnet_train_rollout(grl_fieldnet *net, float lr, float *stats_host);
int grl_fieldnet_train_rollout_grads(grl_fieldnet *net, float *stats_host);
/* which: "actions" "env_actions" (the norm-clipped ones the envs took) "mu" "sigma" (T,B,2) "values" "rewards" "y" "adv" (T,B)
 * "boot" (B) float32; "dones" (T,E) "locust_bins" (T,E,80,2) "agent_bins" "positions" (T,E,10,2) uint8 */
int grl_fieldnet_read_rollout(grl_fieldnet *net, const char *which, void *host, size_t bytes);
int grl_fieldnet_get_optimizer_state(grl_fieldnet *net, float *m_host, float *v_host, int64_t n, int64_t *step_out);
int grl_fieldnet_set_optimizer_state(grl_fieldnet *net, const float *m_host, const float *v_host, int64_t n, int64_t step);
int grl_fieldnet_get_action_counter(grl_fieldnet *net, uint64_t *out);
int grl_fieldnet_set_action_counter(grl_fieldnet *net, uint64_t value);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_FIELDROLLOUT_H */
