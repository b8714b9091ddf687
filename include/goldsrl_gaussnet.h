/* goldsrl_gaussnet.h -- C ABI of the A3C Gaussian agent on the device (SolowWorker / TradeWorker): a GRU trunk shared by a
 * Gaussian policy (mu and sigma towers) and a value head, its device-resident rollout on a Solow or TradeAR1 handle and the A3C
 * update, batched.
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/estimators.py:18-28         rnn_graph_lstm (trunk: GRU 32, dense_temporal 64, static S0 -> 64 -> 32)
 *   fed_gym/agents/a3c/estimators.py:241-334       GaussianPolicyEstimator (mu + sigma towers, loss, RMSProp)
 *   fed_gym/agents/a3c/estimators.py:338-417       ValueEstimator (x -> 256 tanh -> 1, times scale; loss; RMSProp)
 *   fed_gym/agents/a3c/worker.py:69-341,394-442    GaussianWorker, SolowWorker, TradeWorker (acting, window, GAE, update)
 *   scripts/train_solow.py, scripts/train_trade.py the sizes and hyper-parameters
 *
 * Sizes come from the handle: static input = the processed observation (S0), temporal row = the same vector (D = S0), A actions.
 *   Solow                   S0 = D = 2, A = 1     148 547 parameters
 *   TradeAR1 with 2 assets  S0 = D = 5, A = 2     149 285 parameters
 * Any other handle: GRL_E_INVALID.  GRU window R rows (1..20).
 *
 * Flat parameter vector, tf.trainable_variables() order (the policy estimator is created first, the value estimator reuses "shared"):
 *   gru_gates_w[D+32,64] gru_gates_b[64] gru_cand_w[D+32,32] gru_cand_b[32] temporal_w[32,64] temporal_b[64]
 *   static1_w[S0,64] static1_b[64] static2_w[64,32] static2_b[32]                                           (trunk)
 *   mu1_w[96,256] mu1_b mu2_w[256,128] mu2_b mu3_w[128,A] mu3_b
 *   sigma1_w[96,256] sigma1_b sigma2_w[256,128] sigma2_b sigma3_w[128,A] sigma3_b
 *   value1_w[96,256] value1_b value2_w[256,1] value2_b
 * Forward: x = trunk; mu = 5 tanh(mu3(tanh(mu2(relu(mu1 x))))); sigma = sigmoid(sigma3(tanh(sigma2(relu(sigma1 x))))) + 1e-3;
 * value = scale * value2(tanh(value1 x)).
 *
 * Acting, per env e and action a at rollout step t (Philox, oracle/oracle.py:rng_block / normal_pair):
 *   n   = normal_pair(rng_block(seed, e + env_id_offset, action_counter + t, 19, a))[0]
 *   raw = (float)((double)mu[a] + (double)sigma[a] * n)
 * A Solow env gets the stable float32 sigmoid of raw (z = exp(-|raw|); raw >= 0 ? 1/(1+z) : z/(1+z)), a TradeAR1 env tanhf(raw).
 * The raw draw is what is stored and trained on.
 * Window: the last min(k+1, R) processed states of the env's episode (k = its step in the episode), current state last, zero rows
 * after; weight 1 iff k >= R-1 (the worker records a transition only then).  The window restarts at every reset.
 * Returns: GAE on the raw rewards, cut at episode ends.  The value behind a finished episode is 0 (always_bootstrap = 0) or the
 * value net's prediction for the terminal observation under the window that ends in it (always_bootstrap = 1).  The end of the
 * rollout bootstraps from the observation after the last step; if that step ended an episode, the rule above applies instead.
 * Losses, sums over the weighted samples times grad_mult: policy = sum_a nll(raw_a; mu_a, sigma_a) * adv (adv already / scale),
 * value = 0.5 (v - target)^2 / scale; the entropy mean (0.5 + 0.5 log 2 pi + log sigma, weighted) is reported only.
 * Update: policy and value gradients, each clipped to clip_norm on its own, each to its own RMSProp (ms <- rho ms + (1-rho) g^2,
 * w <- w - lr g / sqrt(ms + eps), ms starts at 1): params <- (params - step_p) - step_v.
 * lr = lr0 * decay_rate^(global_step / decay_steps) with the global step before the update; the global step advances by 2.
 * Greedy acting (run_n_steps(stochastic=False) / get_greedy_action, worker.py:180-230): grl_anet_set_greedy(net, 1) makes
 * grl_anet_rollout draw nothing -- raw = mu exactly, the env gets the same sigmoid / tanh of it, the action counter stands still.
 * Greedy evaluation (PolicyMonitor.eval_once, fed_gym/agents/a3c/policy_monitor.py:42-96): grl_anet_eval plays whole greedy
 * episodes of every env in ONE kernel launch: a workgroup keeps 64 envs for the episode and runs per step the trunk, the mu tower
 * (the sigma and value towers are not evaluated), the action, the env step and the window rule -- the device functions the
 * per-step path runs, so it reproduces a greedy grl_anet_rollout bit for bit up to each env's first done.  The evaluation feeds no
 * episode records (grl_episodes_*): its totals and lengths are read with grl_anet_read_eval.  These three functions are declared
 * in goldsrl_gausseval.h, which this header includes.
 * Conventions as in goldsrl.h.
 */
#ifndef GOLDSRL_GAUSSNET_H
#define GOLDSRL_GAUSSNET_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grl_anet_config {
    int32_t struct_size;
    int32_t rnn_length;        /* R: the worker's max_seq_length (scripts/train_solow.py: 5, train_trade.py: 20); 1..20 */
    int32_t max_samples;       /* largest n of one grl_anet_predict / grl_anet_train call (host staging) */
    int32_t lr_decay_steps;    /* 100 000 (estimators.py:319-321) */
    int32_t always_bootstrap;  /* 0 (train_trade.py:119) or 1 (train_solow.py:133).  Solow handles require 1: a Solow episode ends
                                  only at the step cap, never in a terminal state.  TradeAR1 handles require 0. */
    float scale;               /* value scale (1; SolowWorker: 100) */
    float gamma;               /* 0.99 */
    float gae_lambda;          /* 0.96 (worker.py:87) */
    float clip_norm;           /* 40, per gradient */
    float rms_decay;           /* 0.99 */
    float rms_epsilon;         /* 0.1 */
    float lr_decay_rate;       /* 0.96, not staircase */
} grl_anet_config;

typedef struct grl_anet grl_anet;

enum { GRL_ANET_POLICY = 0, GRL_ANET_VALUE = 1 };

int grl_anet_config_default(grl_anet_config *cfg);
/* h must be an ENV_SOLOW handle, or an ENV_TRADE handle with 2 assets (GRL_E_INVALID otherwise, and for an always_bootstrap the
 * handle's env does not take).  Parameters start at zero: set them with grl_anet_set_params.  The windows live in the net, not in
 * a checkpoint: a new net starts every env's window at its current observation, and every rollout restarts the window of an env
 * the handle has just reset (elapsed 0). */
int grl_anet_create(grl_handle *h, const grl_anet_config *cfg, grl_anet **out);
int grl_anet_destroy(grl_anet *net);
const char *grl_anet_last_error(const grl_anet *net);
int64_t grl_anet_num_params(const grl_anet *net);
int grl_anet_set_params(grl_anet *net, const float *host, int64_t n);
int grl_anet_get_params(grl_anet *net, float *host, int64_t n);
/* gradient of the last grl_anet_train / grl_anet_train_rollout before clipping, full length: which = GRL_ANET_POLICY (value blocks
 * 0) or GRL_ANET_VALUE (mu and sigma blocks 0) */
int grl_anet_get_grads(grl_anet *net, int32_t which, float *host, int64_t n);
/* both RMSProp ms vectors (full length; entries a gradient never reaches stay 1) and the global step */
int grl_anet_get_optimizer_state(grl_anet *net, float *ms_policy, float *ms_value, int64_t n, int64_t *global_step);
int grl_anet_set_optimizer_state(grl_anet *net, const float *ms_policy, const float *ms_value, int64_t n, int64_t global_step);
int grl_anet_get_action_counter(grl_anet *net, uint64_t *out);
int grl_anet_set_action_counter(grl_anet *net, uint64_t value);

/* HOST arrays: states (n,S0), windows (n,R,D); outputs mu, sigma (n,A), values (n) (any may be NULL).  Synchronous. */
int grl_anet_predict(grl_anet *net, int32_t n, const float *states, const float *windows, float *mu, float *sigma, float *values);
/* One update on HOST samples: raw (n,A) (the untransformed Gaussian draw), adv (already / scale), targets, weights (n) or NULL
 * (all 1).  Gradients are grad_mult * the sums over the samples.  apply_update = 0: gradients and stats only.
 * stats_host (6): policy loss, value loss (both grad_mult * the weighted sums), entropy mean (weighted), policy norm, value norm
 * (pre-clip), lr used. */
int grl_anet_train(grl_anet *net, int32_t n, const float *states, const float *windows, const float *raw, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host);
/* T steps of every env of the handle, all on the device: forward + draw, env step (auto-reset, episode records), window update;
 * then the bootstrap value passes and the worker's GAE.  Async. */
int grl_anet_rollout(grl_anet *net, int32_t T);
/* the update on the last rollout: grad_mult = 1/E (each env is one A3C worker; the gradient is averaged over them) */
int grl_anet_train_rollout(grl_anet *net, float lr0, float *stats_host);
/* "states" (T,E,S0) "windows" (T,E,R,D) "raw" "mu" "sigma" (T,E,A) "values" "rewards" "dones" "weights" "adv" "targets" (T,E)
 * "actions" (T,E,A): what each env was stepped with (the sigmoid or tanh of raw)
 * "term_values" (T,E): the value behind the episode a step ended (0 where none ended, and everywhere with always_bootstrap 0)
 * "term_states" (T,E,S0) "term_windows" (T,E,R,D): its inputs, defined only where dones != 0; they exist with always_bootstrap 1
 * only (GRL_E_STATE otherwise)
 * "boot" (E): the value behind the last step: of the next observation, or term_values[T-1] where that step ended an episode */
int grl_anet_read_rollout(grl_anet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif

#include "goldsrl_gausseval.h" /* greedy acting and the one-launch greedy evaluation of the same net */

#endif /* GOLDSRL_GAUSSNET_H */
