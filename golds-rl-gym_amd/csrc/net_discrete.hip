// The A3C discrete savings-grid agent on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-28,155-238,338-417 and
// GridSolowWorker, fed_gym/agents/a3c/worker.py:69-341,343-391): the GRU trunk shared by a softmax policy over K savings rates and
// a value head, the device-resident rollout on a Solow handle and the A3C update in batched form (include/goldsrl_discretenet.h).
//
// 90 561 + 129 K parameters.  The third client of the A3C nets' shared code: the trunk, the LDS layout, the GEMMs, the window rules,
// the GAE and the update are net_a3c_core.inc's, the host scaffold and the rollout loop net_a3c_host.h's.  The towers, the softmax
// head, the sampler, the arg-max, the loss behind them and the host calls are the softmax-grid head's (net_a3c_grid.inc,
// net_a3c_grid_host.h), which this net instantiates with ONE output over a 2-wide observation: the grid trader (net_gridtrade.hip)
// is the same head with two.  What is this net's own: the sizes below, the Solow handle's refusals and terminal-pass buffers, and
//   eval      whole greedy episodes in one launch (net_discrete_eval.inc): a workgroup keeps its 64 envs, probs tower only
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/goldsrl_discretenet.h"
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "flat_env_dev.h"

namespace grl {

enum : uint32_t { RS_GRID_ACTION = 20 };    // next to RS_GATED_ACTION = 18 (net_gated.hip) and RS_GAUSS_ACTION = 19 (net_gauss.hip)
constexpr int A3C_DPAD = 2;   // Solow's processed observation
constexpr bool A3C_PAD_LAST = true;
constexpr int GRID_D = 2;     // S0 = D = 2
constexpr int GRID_O = 1;     // one softmax: the savings rate
constexpr int GRID_KMAX = 64; // most grid points
constexpr uint32_t GRID_RS = RS_GRID_ACTION;

#include "net_a3c_core.inc"
#include "net_a3c_grid.inc"

__global__ __launch_bounds__(256) void disc_forward_kernel(GridArgs a) {
    extern __shared__ float lds[];
    grid_forward(a, lds);
}

__global__ __launch_bounds__(256, 1) void disc_backward_kernel(GridArgs a) {
    extern __shared__ float lds[];
    grid_backward(a, lds);
}

#include "net_discrete_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"
#include "net_a3c_grid_host.h"

struct grl_dnet : grl::GridNetBase {
    grl_dnet_config cfg;
};

namespace grl {

struct DiscEnv {
    static constexpr auto forward = disc_forward_kernel, backward = disc_backward_kernel;
    static constexpr auto eval = disc_eval_kernel;
    static const float *obs(grl_handle *h) { return h->so.obs; }
    static int step(grl_handle *h, const float *act, float *term_obs) { return solow_launch_step(h, act, term_obs); }
    static int reset(grl_handle *h) { return solow_launch_reset(h, h->done_list, h->done_count, h->E, true); }      // with the tape draw
    static SolowParams params(grl_handle *h) { return solow_params(h); }
};

}  // namespace grl

using namespace grl;

extern "C" {

int grl_dnet_config_default(grl_dnet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_dnet_config);
    cfg->rnn_length = 5; cfg->max_samples = 8192; cfg->lr_decay_steps = 100000; cfg->always_bootstrap = 1; cfg->num_choices = 51;
    cfg->scale = 1.f; cfg->gamma = 0.99f; cfg->gae_lambda = 0.96f; cfg->clip_norm = 40.f;
    cfg->rms_decay = 0.99f; cfg->rms_epsilon = 0.1f; cfg->lr_decay_rate = 0.96f;
    cfg->grid_lb = 0.01; cfg->grid_ub = 0.99;
    return GRL_OK;
}

int grl_dnet_create(grl_handle *h, const grl_dnet_config *cfg, grl_dnet **out) {
    return a3c_create(
        "grl_dnet_create", h, cfg, out,
        [&](const char *range) -> const char * {
            if (h->cfg.env_kind != GRL_ENV_SOLOW) return "the savings-grid agent needs a Solow handle";
            if (range) return range;
            if (cfg->num_choices < 2 || cfg->num_choices > GRID_KMAX || !(cfg->grid_lb < cfg->grid_ub)) return "num_choices 2..64, grid_lb < grid_ub";
            return cfg->always_bootstrap != 1 ? "a Solow handle needs always_bootstrap = 1" : nullptr;
        },
        [&](grl_dnet *n, A3cGrow &Al) {
            n->S0 = n->D = GRID_D; n->K = cfg->num_choices;
            n->off = grid_offsets(n->K);
            const size_t ms = cfg->max_samples, E = h->E, K = n->K, W = (size_t)cfg->rnn_length * GRID_D;
            n->ro_bufs = {a3c_buf("probs", &n->ro_probs, K), a3c_buf("choices", &n->ro_choice, 1), a3c_buf("actions", &n->ro_act, 1),
                          a3c_buf("term_values", &n->ro_term_val, 1), a3c_buf("term_states", &n->ro_term_st, GRID_D),
                          a3c_buf("term_windows", &n->ro_term_wn, W)};
            n->ev_bufs = {a3c_buf("choices", &n->ev_choice, 1), a3c_buf("actions", &n->ev_actions, 1)};
            Al(&n->d_choice, ms); Al(&n->d_probs, ms * K); Al(&n->term_obs, E * GRID_D); Al(&n->ev_act, E);
            return (size_t)n->off.total;
        },
        {(const void *)disc_forward_kernel, (const void *)disc_backward_kernel, (const void *)disc_eval_kernel});
}

int grl_dnet_destroy(grl_dnet *n) { return a3c_destroy(n); }
const char *grl_dnet_last_error(const grl_dnet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_dnet_num_params(const grl_dnet *n) { return n ? n->num_params : 0; }
int grl_dnet_set_params(grl_dnet *n, const float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, (float *)host, cnt, true); }
int grl_dnet_get_params(grl_dnet *n, float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, host, cnt, false); }
int grl_dnet_get_grads(grl_dnet *n, int32_t which, float *host, int64_t cnt) { return a3c_get_grads(n, "grl_dnet_get_grads", which, host, cnt); }
int grl_dnet_get_optimizer_state(grl_dnet *n, float *msp, float *msv, int64_t cnt, int64_t *step) { return a3c_get_optimizer_state(n, msp, msv, cnt, step); }
int grl_dnet_set_optimizer_state(grl_dnet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) { return a3c_set_optimizer_state(n, msp, msv, cnt, step); }
int grl_dnet_get_action_counter(grl_dnet *n, uint64_t *out) { return a3c_get_action_counter(n, out); }
int grl_dnet_set_action_counter(grl_dnet *n, uint64_t v) { return a3c_set_action_counter(n, v); }
int grl_dnet_set_greedy(grl_dnet *net, int32_t on) { return a3c_set_greedy(net, on); }

int grl_dnet_predict(grl_dnet *net, int32_t n, const float *states, const float *windows, float *probs, float *values) {
    return grid_predict<DiscEnv>(net, "grl_dnet_predict", n, states, windows, probs, values);
}
int grl_dnet_train(grl_dnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    return grid_train<DiscEnv>(net, "grl_dnet_train", n, states, windows, choices, adv, targets, weights, grad_mult, lr0, apply_update, stats_host);
}
int grl_dnet_rollout(grl_dnet *net, int32_t T) { return grid_rollout<DiscEnv>(net, "grl_dnet_rollout", T); }
int grl_dnet_eval(grl_dnet *net, int32_t max_steps, int32_t trace_steps) { return grid_eval<DiscEnv>(net, "grl_dnet_eval", max_steps, trace_steps); }
int grl_dnet_read_eval(grl_dnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_dnet_read_eval", which, host, bytes); }
int grl_dnet_train_rollout(grl_dnet *net, float lr0, float *stats_host) { return grid_train_rollout<DiscEnv>(net, "grl_dnet_train_rollout", lr0, stats_host); }
int grl_dnet_read_rollout(grl_dnet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_dnet_read_rollout", "", which, host, bytes);
}

}  // extern "C"
