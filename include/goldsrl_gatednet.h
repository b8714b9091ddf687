/* goldsrl_gatednet.h -- C ABI of the Ticker gated trader on the device: a GRU trunk shared by a categorical + per-choice
 * Gaussian policy and a value head, its device-resident rollout on a Ticker handle and the A3C update, batched.
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/estimators.py:18-28         rnn_graph_lstm (trunk: GRU 32, dense_temporal 64, static 7 -> 64 -> 32)
 *   fed_gym/agents/a3c/estimators.py:40-152        DiscreteAndContPolicyEstimator (class + normal towers, loss, RMSProp)
 *   fed_gym/agents/a3c/estimators.py:338-417       ValueEstimator (x -> 256 tanh -> 1, times scale; loss; RMSProp)
 *   fed_gym/agents/a3c/worker.py:191-294,445-494   TickerGatedTraderWorker (acting, window, GAE, update)
 *
 * Sizes are the Ticker env's: 2 assets x 3 choices (0 hold, 1 buy, 2 sell), static input = the processed observation (7), temporal
 * row = its last 4 columns (log prices, volumes), GRU window R rows (1..20).
 *
 * Flat parameter vector, tf.trainable_variables() order (151 123 floats):
 *   gru_gates_w[36,64] gru_gates_b[64] gru_cand_w[36,32] gru_cand_b[32] temporal_w[32,64] temporal_b[64]
 *   static1_w[7,64] static1_b[64] static2_w[64,32] static2_b[32]                                      (trunk: 8 256)
 *   class1_w[96,256] class1_b class2_w[256,128] class2_b class3_w[128,6] class3_b                     (logits: asset-major)
 *   normal1_w[96,256] normal1_b normal2_w[256,128] normal2_b normal3_w[128,12] normal3_b              (asset, choice, {mu, raw sigma})
 *   value1_w[96,256] value1_b value2_w[256,1] value2_b
 *
 * Acting, per env e and asset a at rollout step t (Philox, oracle/oracle.py:rng_block / u01_pair / normal_pair):
 *   u = u01_pair(rng_block(seed, e + env_id_offset, action_counter + t, 18, 2a))[0]
 *   n = normal_pair(rng_block(seed, e + env_id_offset, action_counter + t, 18, 2a + 1))[0]
 *   choice = first c with u < cum[c] (cum = float32 cumsum of probs[a] in index order; compared in float64), else 0
 *   raw = (float)((double)mu[a][choice] + (double)sigma[a][choice] * n); the env gets (float)(1 / (1 + exp(-(double)raw)))
 * Window: the last min(k+1, R) temporal rows of the env's episode (k = its step in the episode), current row last, zero rows
 * after; weight 1 iff k >= R-1 (the worker records a transition only then).  The window restarts at every reset.
 * Update: policy and value gradients (sums over the weighted samples times grad_mult), each clipped to clip_norm on its own, each
 * to its own RMSProp (ms <- rho ms + (1-rho) g^2, w <- w - lr g / sqrt(ms + eps), ms starts at 1): params <- (params - step_p) - step_v.
 * lr = lr0 * decay_rate^(global_step / decay_steps) with the global step before the update; the global step advances by 2.
 * Conventions as in goldsrl.h.  Greedy acting (grl_gnet_set_greedy) and the one-launch greedy evaluation (grl_gnet_eval) are declared
 * in goldsrl_gatedeval.h, which this header includes.
 */
#ifndef GOLDSRL_GATEDNET_H
#define GOLDSRL_GATEDNET_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grl_gnet_config {
    int32_t struct_size;
    int32_t rnn_length;       /* R: the worker's max_seq_length (5; scripts/train_trade.py: 20); 1..20 */
    int32_t max_samples;      /* largest n of one grl_gnet_predict / grl_gnet_train call (host staging) */
    int32_t lr_decay_steps;   /* 100 000 (estimators.py:134-136) */
    float scale;              /* value scale (1) */
    float gamma;              /* 0.99 */
    float gae_lambda;         /* 0.96 (worker.py:87) */
    float clip_norm;          /* 40, per gradient */
    float rms_decay;          /* 0.99 */
    float rms_epsilon;        /* 0.1 */
    float lr_decay_rate;      /* 0.96, not staircase */
} grl_gnet_config;

typedef struct grl_gnet grl_gnet;

enum { GRL_GNET_POLICY = 0, GRL_GNET_VALUE = 1 };

int grl_gnet_config_default(grl_gnet_config *cfg);
/* h must be an ENV_TICKER handle (GRL_E_INVALID otherwise).  Parameters start at zero: set them with grl_gnet_set_params.  The
 * windows live in the net, not in a checkpoint: a new net starts every env's window at its current observation, and every
 * rollout restarts the window of an env the handle has just reset (elapsed 0). */
int grl_gnet_create(grl_handle *h, const grl_gnet_config *cfg, grl_gnet **out);
int grl_gnet_destroy(grl_gnet *net);
const char *grl_gnet_last_error(const grl_gnet *net);
int64_t grl_gnet_num_params(const grl_gnet *net);
int grl_gnet_set_params(grl_gnet *net, const float *host, int64_t n);
int grl_gnet_get_params(grl_gnet *net, float *host, int64_t n);
/* gradient of the last grl_gnet_train / grl_gnet_train_rollout before clipping, full length: which = GRL_GNET_POLICY (value blocks
 * 0) or GRL_GNET_VALUE (class and normal blocks 0) */
int grl_gnet_get_grads(grl_gnet *net, int32_t which, float *host, int64_t n);
/* both RMSProp ms vectors (full length; entries a gradient never reaches stay 1) and the global step */
int grl_gnet_get_optimizer_state(grl_gnet *net, float *ms_policy, float *ms_value, int64_t n, int64_t *global_step);
int grl_gnet_set_optimizer_state(grl_gnet *net, const float *ms_policy, const float *ms_value, int64_t n, int64_t global_step);
int grl_gnet_get_action_counter(grl_gnet *net, uint64_t *out);
int grl_gnet_set_action_counter(grl_gnet *net, uint64_t value);

/* HOST arrays: states (n,7), windows (n,R,4); outputs probs, mu, sigma (n,2,3), values (n) (any may be NULL).  Synchronous. */
int grl_gnet_predict(grl_gnet *net, int32_t n, const float *states, const float *windows, float *probs, float *mu, float *sigma,
                     float *values);
/* One update on HOST samples: choices int32 (n,2), raw (n,2) (the untransformed Gaussian draw), adv (already / scale), targets,
 * weights (n) or NULL (all 1).  Gradients are grad_mult * the sums over the samples.  apply_update = 0: gradients and stats only.
 * stats_host (6): policy loss, value loss (both grad_mult * the weighted sums), entropy mean (weighted), policy norm, value norm
 * (pre-clip), lr used. */
int grl_gnet_train(grl_gnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *raw,
                   const float *adv, const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update,
                   float *stats_host);
/* T steps of every env of the handle, all on the device: forward + draw, Ticker step (auto-reset, episode records), window
 * update; then the bootstrap value pass and the worker's GAE.  Async. */
int grl_gnet_rollout(grl_gnet *net, int32_t T);
/* the update on the last rollout: grad_mult = 1/E (each env is one A3C worker; the gradient is averaged over them) */
int grl_gnet_train_rollout(grl_gnet *net, float lr0, float *stats_host);
/* "states" (T,E,7) "windows" (T,E,R,4) "choices" (T,E,2) int32 "raw" (T,E,2) "probs" "mu" "sigma" (T,E,2,3) "values" "rewards"
 * "dones" "weights" "adv" "targets" (T,E) "actions" (T,E,4) (what the env was stepped with: both choices, both fractions)
 * "boot" (E) (0 behind a finished episode) */
int grl_gnet_read_rollout(grl_gnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif

#include "goldsrl_gatedeval.h" /* greedy acting and the one-launch greedy evaluation of the same net */

#endif /* GOLDSRL_GATEDNET_H */
