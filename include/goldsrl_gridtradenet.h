/* goldsrl_gridtradenet.h -- C ABI of the A3C grid trader on the device: DiscretePolicyEstimator with num_outputs = 2 on a 2-asset
 * TradeAR1 handle.  The GRU trunk of the Gaussian agent shared by one softmax over K grid points PER ASSET and a value head, its
 * device-resident rollout, the A3C update, batched, and the one-launch greedy evaluation.
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/estimators.py:18-28         rnn_graph_lstm (trunk: GRU 32, dense_temporal 64, static S0 -> 64 -> 32)
 *   fed_gym/agents/a3c/estimators.py:155-238       DiscretePolicyEstimator(num_outputs, num_choices, ..): logits num_outputs *
 *                                                  num_choices, reshaped (-1, num_outputs, num_choices), one softmax per output
 *   fed_gym/agents/a3c/estimators.py:338-417       ValueEstimator (x -> 256 tanh -> 1, times scale; loss; RMSProp)
 *   fed_gym/agents/a3c/worker.py:69-341            GaussianWorker's loop and update
 *
 * What has no counterpart.  The reference ships and tests the estimator with several outputs (estimators_tests.py:240 builds it
 * with n_assets outputs) but has NO Trade grid worker.  The agent here is the composition of two workers it does have:
 *   from TradeWorker (worker.py:418-442)      the processed state (log(cash + 1e-4), log(q + 1), log p), R = 20,
 *                                             always_bootstrap = 0 and the value scale
 *   from GridSolowWorker (worker.py:343-391)  acting and update: the cumulative-sum draw per output, idx_to_grid =
 *                                             np.linspace(lb, ub, K), actions.reshape((-1, num_outputs)), advantages / scale
 *   the grid is on [-1, 1], the env's action box
 * Why: the Gaussian trader steps the env with tanh(raw), which never reaches +-1 and holds at exactly 0 with probability zero,
 * while the yardsticks of TradeAR1 play exactly those actions -- the foresight plan is bang-bang in {-1, 0, 1} per asset and the
 * attainable optimum (goldsrl_tradedp.h) chooses from a 17-point grid per action component.  K = 17 on [-1, 1] is that grid.
 *
 * Only ENV_TRADE handles with 2 assets: S0 = D = 5, O = num_outputs = 2 (one per asset), K = num_choices grid points, 2..48: the
 * O * K logits share the 96 rows the device's layout has for them.
 *   91 041 + 258 K parameters: 95 427 at K = 17.
 * GRU window R rows (1..20).
 *
 * Flat parameter vector, tf.trainable_variables() order:
 *   gru_gates_w[D+32,64] gru_gates_b[64] gru_cand_w[D+32,32] gru_cand_b[32] temporal_w[32,64] temporal_b[64]
 *   static1_w[S0,64] static1_b[64] static2_w[64,32] static2_b[32]                                           (trunk)
 *   probs1_w[96,256] probs1_b probs2_w[256,128] probs2_b probs3_w[128,O*K] probs3_b[O*K]
 *   value1_w[96,256] value1_b value2_w[256,1] value2_b
 * Column o * K + j of probs3 is output o, choice j: the row-major reshape.
 * Forward: x = trunk; logits = probs3(relu(probs2(relu(probs1 x)))); probs[o] = softmax(logits[o*K .. o*K+K)) in float32,
 * max-subtracted, the sum taken in index order; value = scale * value2(tanh(value1 x)).
 *
 * Acting, per env e at rollout step t (Philox, oracle/oracle.py:rng_block / u01_pair; stream id 21), ONE block per env and step:
 *   u_0, u_1 = u01_pair(rng_block(seed, e + env_id_offset, action_counter + t, 21, 0))       first uniform: output 0, second: output 1
 *   c_o[j]   = the float32 cumulative sum of probs[o] in index order
 *   choice_o = the first j with u_o < (double)c_o[j], 0 if there is none          ((u < cum_probs).argmax(), worker.py:223-227)
 *   action_o = (float)grid[choice_o], grid = np.linspace(grid_lb, grid_ub, K) in float64: grid_lb + j * ((grid_ub - grid_lb) /
 *              (K - 1)), the last point grid_ub exactly
 * The centre.  With an odd K on a symmetric grid (grid_lb = -grid_ub) the agent must be able to hold: the middle point must be
 * exactly 0.0f.  Nothing special-cases it: grl_gtnet_create computes it by the formula above and refuses the configuration
 * (GRL_E_INVALID) if it is not.  On [-1, 1] it is exactly 0 for every odd K in 3..47.
 * The int32 choices are what is stored and trained on; the env is stepped with the grid values.
 * Window, weights, returns (GAE on the raw rewards cut at episode ends; a TradeAR1 episode ends terminally, so nothing is
 * bootstrapped behind one: always_bootstrap = 0, goldsrl_gaussnet.h) and the update are the Gaussian agent's.
 * Losses, sums over the weighted samples with c = grad_mult * weight, cp = c * adv (adv already / scale):
 *   policy  cp * sum_o -log(p[o][choice_o] + 1e-7)      (1e-7 is the Keras epsilon, and the gradient carries it:
 *           d/dlogit[o][j] = cp * p[o][choice_o] / (p[o][choice_o] + 1e-7) * (p[o][j] - [j == choice_o]))
 *   value   c * 0.5 (v - target)^2 / scale
 *   the entropy, per sample the mean over o of -sum_j p[o][j] log(p[o][j] + 1e-7) (estimators.py:206), weighted mean over the
 *   samples, is reported only: it is no part of the loss
 * Update: policy and value gradients, each clipped to clip_norm on its own, each to its own RMSProp; the global step advances by 2.
 *
 * Greedy acting and evaluation.  As for the savings-grid agent (goldsrl_discreteeval.h) the reference's greedy path cannot run, and
 * the evident intention is taken: per output, choice = the first index of the largest float32 probability (np.argmax), action =
 * grid[choice].  Nothing is drawn and the action counter stands still.  grl_gtnet_eval is ONE kernel launch: a workgroup of 4 waves
 * keeps 64 envs for the whole episode and runs per step the trunk, the probs tower (the value tower is not evaluated), both
 * softmaxes and arg-maxes, the env step, the window rule and the float64 reward sum.  These are the device functions the per-step
 * path (grl_gtnet_rollout with greedy on) runs, so the two agree bit for bit up to each env's first done.  The evaluation feeds no
 * episode records (grl_episodes_*).
 * Conventions as in goldsrl.h.
 */
#ifndef GOLDSRL_GRIDTRADENET_H
#define GOLDSRL_GRIDTRADENET_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grl_gtnet_config {
    int32_t struct_size;
    int32_t rnn_length;        /* R: the worker's max_seq_length; 1..20, default 20 (TradeWorker) */
    int32_t max_samples;       /* largest n of one grl_gtnet_predict / grl_gtnet_train call (host staging) */
    int32_t lr_decay_steps;    /* 100 000 (estimators.py:223-225) */
    int32_t always_bootstrap;  /* 0, and it must be: a TradeAR1 episode ends in a terminal state */
    int32_t num_choices;       /* K: grid points per output, 2..48; 17 (the attainable optimum's action grid) */
    int32_t num_outputs;       /* O: must equal the handle's asset count, 2 today */
    float scale;               /* value scale; 1 */
    float gamma;               /* 0.99 */
    float gae_lambda;          /* 0.96 (worker.py:87) */
    float clip_norm;           /* 40, per gradient */
    float rms_decay;           /* 0.99 */
    float rms_epsilon;         /* 0.1 */
    float lr_decay_rate;       /* 0.96, not staircase */
    double grid_lb;            /* -1: the env's action box.  float64, as np.linspace computes the grid */
    double grid_ub;            /* 1; grid_lb < grid_ub */
} grl_gtnet_config;

typedef struct grl_gtnet grl_gtnet;

enum { GRL_GTNET_POLICY = 0, GRL_GTNET_VALUE = 1 };

int grl_gtnet_config_default(grl_gtnet_config *cfg);
/* GRL_E_INVALID, with the reason in grl_last_error(h): h is no ENV_TRADE handle; num_outputs differs from the handle's asset count
 * or that is not 2 (both numbers are in the message); num_choices outside 2..48; always_bootstrap != 0; an odd symmetric grid
 * whose centre is not 0.0f.  Parameters start at zero: set them with grl_gtnet_set_params. */
int grl_gtnet_create(grl_handle *h, const grl_gtnet_config *cfg, grl_gtnet **out);
int grl_gtnet_destroy(grl_gtnet *net);
const char *grl_gtnet_last_error(const grl_gtnet *net);
int64_t grl_gtnet_num_params(const grl_gtnet *net);
int grl_gtnet_set_params(grl_gtnet *net, const float *host, int64_t n);
int grl_gtnet_get_params(grl_gtnet *net, float *host, int64_t n);
/* gradient of the last grl_gtnet_train / grl_gtnet_train_rollout before clipping, full length: which = GRL_GTNET_POLICY (value
 * blocks 0) or GRL_GTNET_VALUE (probs blocks 0) */
int grl_gtnet_get_grads(grl_gtnet *net, int32_t which, float *host, int64_t n);
/* both RMSProp ms vectors (full length; entries a gradient never reaches stay 1) and the global step */
int grl_gtnet_get_optimizer_state(grl_gtnet *net, float *ms_policy, float *ms_value, int64_t n, int64_t *global_step);
int grl_gtnet_set_optimizer_state(grl_gtnet *net, const float *ms_policy, const float *ms_value, int64_t n, int64_t global_step);
int grl_gtnet_get_action_counter(grl_gtnet *net, uint64_t *out);
int grl_gtnet_set_action_counter(grl_gtnet *net, uint64_t value);

/* HOST arrays: states (n,5), windows (n,R,5); outputs probs (n,O,K), values (n) (either may be NULL).  Synchronous. */
int grl_gtnet_predict(grl_gtnet *net, int32_t n, const float *states, const float *windows, float *probs, float *values);
/* One update on HOST samples: choices (n,O) int32 in [0, K) (GRL_E_INVALID otherwise), adv (already / scale), targets, weights (n)
 * or NULL (all 1).  Gradients are grad_mult * the sums over the samples.  apply_update = 0: gradients and stats only.
 * stats_host (6): policy loss, value loss (both grad_mult * the weighted sums), entropy mean (weighted), policy norm, value norm
 * (pre-clip), lr used. */
int grl_gtnet_train(grl_gtnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                    const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host);
/* T steps of every env of the handle, all on the device: forward + draws, env step (auto-reset, episode records), window update;
 * then the bootstrap value pass and the worker's GAE.  Async. */
int grl_gtnet_rollout(grl_gtnet *net, int32_t T);
/* the update on the last rollout: grad_mult = 1/E (each env is one A3C worker; the gradient is averaged over them) */
int grl_gtnet_train_rollout(grl_gtnet *net, float lr0, float *stats_host);
/* "states" (T,E,5) "windows" (T,E,R,5) "probs" (T,E,O,K) float32; "choices" (T,E,O) int32; "actions" (T,E,O): the grid values each
 * env was stepped with; "values" "rewards" "dones" "weights" "adv" "targets" (T,E); "boot" (E). */
int grl_gtnet_read_rollout(grl_gtnet *net, const char *which, void *host, size_t bytes);

/* on != 0: grl_gtnet_rollout acts greedily -- "choices" are the arg-maxes of "probs" (first index on ties), nothing is drawn and
 * the action counter does not advance; windows, records, GAE and grl_gtnet_train_rollout as ever.  The default is 0. */
int grl_gtnet_set_greedy(grl_gtnet *net, int32_t on);
/* Greedy episodes of every env of the handle, from the handle's CURRENT state (the caller resets first, as eval_once does).
 * Every env's window restarts at its current observation and follows the rollout's window rule.  An env stops at its first done;
 * the call ends when every env has stopped or after max_steps steps (max_steps >= 1, GRL_E_INVALID otherwise; trace_steps >= 0,
 * capped at max_steps).  Async on the handle's stream.  Afterwards the whole handle is reset as by grl_reset, and the next rollout
 * starts every env's window anew.  Parameters, optimizer state, the action counter, the last rollout's buffers and the handle's
 * episode records are untouched. */
int grl_gtnet_eval(grl_gtnet *net, int32_t max_steps, int32_t trace_steps);
/* "total_reward" (E) float64: the float32 step rewards added in step order in float64
 * "length" (E) int32; "finished" (E) uint8: 0 where max_steps cut the episode
 * trace, the first S = min(trace_steps, steps played) steps (steps played = the longest episode), defined up to each env's own end:
 * "states" (S,E,5) float32, "choices" (S,E,O) int32, "actions" (S,E,O) "rewards" (S,E) "dones" (S,E) float32.  Synchronises.
 * GRL_E_STATE before the first grl_gtnet_eval. */
int grl_gtnet_read_eval(grl_gtnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_GRIDTRADENET_H */
