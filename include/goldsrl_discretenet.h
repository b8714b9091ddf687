/* goldsrl_discretenet.h -- C ABI of the A3C discrete savings-grid agent on the device (GridSolowWorker on DiscretePolicyEstimator):
 * the GRU trunk of the Gaussian agent shared by a softmax policy over K savings rates and a value head, its device-resident rollout
 * on a Solow handle and the A3C update, batched.
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/a3c/estimators.py:18-28         rnn_graph_lstm (trunk: GRU 32, dense_temporal 64, static S0 -> 64 -> 32)
 *   fed_gym/agents/a3c/estimators.py:155-238       DiscretePolicyEstimator (probs tower, softmax, loss, RMSProp)
 *   fed_gym/agents/a3c/estimators.py:338-417       ValueEstimator (x -> 256 tanh -> 1, times scale; loss; RMSProp)
 *   fed_gym/agents/a3c/worker.py:69-341,343-391    GaussianWorker's loop and update as GridSolowWorker runs them
 *
 * Only ENV_SOLOW handles: S0 = D = 2, one output (Solow has one action) with K = num_choices grid points, 2..64.
 *   90 561 + 129 K parameters: 97 140 at K = 51, 90 948 at K = 3.
 * GRU window R rows (1..20).
 *
 * Flat parameter vector, tf.trainable_variables() order:
 *   gru_gates_w[D+32,64] gru_gates_b[64] gru_cand_w[D+32,32] gru_cand_b[32] temporal_w[32,64] temporal_b[64]
 *   static1_w[S0,64] static1_b[64] static2_w[64,32] static2_b[32]                                           (trunk)
 *   probs1_w[96,256] probs1_b probs2_w[256,128] probs2_b probs3_w[128,K] probs3_b
 *   value1_w[96,256] value1_b value2_w[256,1] value2_b
 * Forward: x = trunk; logits = probs3(relu(probs2(relu(probs1 x)))) -- both hidden layers ReLU; probs = softmax(logits) in float32,
 * max-subtracted, the sum taken in index order; value = scale * value2(tanh(value1 x)).
 *
 * Acting, per env e at rollout step t (Philox, oracle/oracle.py:rng_block / u01_pair; stream id 20):
 *   u      = u01_pair(rng_block(seed, e + env_id_offset, action_counter + t, 20, 0))[0]
 *   c[i]   = the float32 cumulative sum of probs in index order
 *   choice = the first i with u < (double)c[i], 0 if there is none          ((u < cum_probs).argmax(), worker.py:223-227)
 *   action = (float)grid[choice], grid = np.linspace(grid_lb, grid_ub, K) in float64: grid_lb + i * ((grid_ub - grid_lb) / (K - 1)),
 *            the last point grid_ub exactly
 * The int32 choice is what is stored and trained on; the env is stepped with the grid value.
 * Window, weights, returns (GAE on the raw rewards cut at episode ends, the terminal bootstrap of always_bootstrap = 1) and the
 * update are the Gaussian agent's (goldsrl_gaussnet.h).
 * Losses, sums over the weighted samples with c = grad_mult * weight:
 *   policy  c * adv * -log(p_choice + 1e-7)      (adv already / scale; 1e-7 is the Keras epsilon, and the gradient carries it:
 *           d/dlogit_j = c * adv * p_choice / (p_choice + 1e-7) * (p_j - [j == choice]))
 *   value   c * 0.5 (v - target)^2 / scale
 *   the entropy -sum_j p_j log(p_j + 1e-7), weighted mean, is reported only: it is no part of the loss (estimators.py:206-212)
 * Update: policy and value gradients, each clipped to clip_norm on its own, each to its own RMSProp; the global step advances by 2.
 * Greedy acting and greedy evaluation: goldsrl_discreteeval.h, which this header includes.
 * Conventions as in goldsrl.h.
 */
#ifndef GOLDSRL_DISCRETENET_H
#define GOLDSRL_DISCRETENET_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grl_dnet_config {
    int32_t struct_size;
    int32_t rnn_length;        /* R: the worker's max_seq_length; 1..20, default 5 */
    int32_t max_samples;       /* largest n of one grl_dnet_predict / grl_dnet_train call (host staging) */
    int32_t lr_decay_steps;    /* 100 000 (estimators.py:223-225) */
    int32_t always_bootstrap;  /* 1, and it must be: a Solow episode ends only at the step cap, never in a terminal state */
    int32_t num_choices;       /* K: grid points, 2..64; 51 (GridSolowWorker's n_grid) */
    float scale;               /* value scale; 1 (GridSolowWorker's default) */
    float gamma;               /* 0.99 */
    float gae_lambda;          /* 0.96 (worker.py:87) */
    float clip_norm;           /* 40, per gradient */
    float rms_decay;           /* 0.99 */
    float rms_epsilon;         /* 0.1 */
    float lr_decay_rate;       /* 0.96, not staircase */
    double grid_lb;            /* 0.01: the lowest savings rate.  float64, as np.linspace computes the grid */
    double grid_ub;            /* 0.99: the highest; grid_lb < grid_ub */
} grl_dnet_config;

typedef struct grl_dnet grl_dnet;

enum { GRL_DNET_POLICY = 0, GRL_DNET_VALUE = 1 };

int grl_dnet_config_default(grl_dnet_config *cfg);
/* h must be an ENV_SOLOW handle (GRL_E_INVALID otherwise, and for always_bootstrap != 1).  Parameters start at zero: set them with
 * grl_dnet_set_params.  The windows live in the net, not in a checkpoint (goldsrl_gaussnet.h). */
int grl_dnet_create(grl_handle *h, const grl_dnet_config *cfg, grl_dnet **out);
int grl_dnet_destroy(grl_dnet *net);
const char *grl_dnet_last_error(const grl_dnet *net);
int64_t grl_dnet_num_params(const grl_dnet *net);
int grl_dnet_set_params(grl_dnet *net, const float *host, int64_t n);
int grl_dnet_get_params(grl_dnet *net, float *host, int64_t n);
/* gradient of the last grl_dnet_train / grl_dnet_train_rollout before clipping, full length: which = GRL_DNET_POLICY (value blocks
 * 0) or GRL_DNET_VALUE (probs blocks 0) */
int grl_dnet_get_grads(grl_dnet *net, int32_t which, float *host, int64_t n);
/* both RMSProp ms vectors (full length; entries a gradient never reaches stay 1) and the global step */
int grl_dnet_get_optimizer_state(grl_dnet *net, float *ms_policy, float *ms_value, int64_t n, int64_t *global_step);
int grl_dnet_set_optimizer_state(grl_dnet *net, const float *ms_policy, const float *ms_value, int64_t n, int64_t global_step);
int grl_dnet_get_action_counter(grl_dnet *net, uint64_t *out);
int grl_dnet_set_action_counter(grl_dnet *net, uint64_t value);

/* HOST arrays: states (n,2), windows (n,R,2); outputs probs (n,K), values (n) (either may be NULL).  Synchronous. */
int grl_dnet_predict(grl_dnet *net, int32_t n, const float *states, const float *windows, float *probs, float *values);
/* One update on HOST samples: choices (n) int32 in [0, K) (GRL_E_INVALID otherwise), adv (already / scale), targets, weights (n) or
 * NULL (all 1).  Gradients are grad_mult * the sums over the samples.  apply_update = 0: gradients and stats only.
 * stats_host (6): policy loss, value loss (both grad_mult * the weighted sums), entropy mean (weighted), policy norm, value norm
 * (pre-clip), lr used. */
int grl_dnet_train(grl_dnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host);
/* T steps of every env of the handle, all on the device: forward + draw, env step (auto-reset, episode records), window update;
 * then the bootstrap value passes and the worker's GAE.  Async. */
int grl_dnet_rollout(grl_dnet *net, int32_t T);
/* the update on the last rollout: grad_mult = 1/E (each env is one A3C worker; the gradient is averaged over them) */
int grl_dnet_train_rollout(grl_dnet *net, float lr0, float *stats_host);
/* "states" (T,E,2) "windows" (T,E,R,2) "probs" (T,E,K) float32; "choices" (T,E) int32; "actions" (T,E): the grid value each env was
 * stepped with; "values" "rewards" "dones" "weights" "adv" "targets" "term_values" (T,E); "term_states" (T,E,2) "term_windows"
 * (T,E,R,2), defined where dones != 0; "boot" (E) -- as the Gaussian net's, with "probs" and "choices" in place of "mu", "sigma"
 * and "raw". */
int grl_dnet_read_rollout(grl_dnet *net, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif

#include "goldsrl_discreteeval.h" /* greedy acting and the one-launch greedy evaluation of the same net */

#endif /* GOLDSRL_DISCRETENET_H */
