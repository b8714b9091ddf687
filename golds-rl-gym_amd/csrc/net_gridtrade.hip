// The A3C grid trader on gfx950: the reference's DiscretePolicyEstimator with num_outputs = 2 (fed_gym/agents/a3c/estimators.py:
// 18-28,155-238,338-417) on a 2-asset TradeAR1 handle -- the GRU trunk shared by one softmax over K grid points PER ASSET and a value
// head, the device-resident rollout and the A3C update in batched form (include/goldsrl_gridtradenet.h, which says how the agent
// is composed from TradeWorker and GridSolowWorker: the reference has no Trade grid worker).
//
// 91 041 + 258 K parameters.  The fourth client of the A3C nets' shared code: the trunk, the LDS layout, the GEMMs, the window
// rules, the GAE and the update are net_a3c_core.inc's, the host scaffold and the rollout loop net_a3c_host.h's.  The towers, the
// per-output softmax head (wave o owns output o; one Philox block per env and step, its first uniform for output 0, its second for
// output 1), the loss and the host calls are the softmax-grid head's (net_a3c_grid.inc, net_a3c_grid_host.h), which this net
// instantiates with TWO outputs over a 5-wide observation: the savings-grid net (net_discrete.hip) is the same head with one.
// What is this net's own: the sizes below, the TradeAR1 handle's refusals (no terminal-pass buffers: episodes end terminally), and
//   eval     whole greedy episodes in one launch (net_gridtrade_eval.inc): a workgroup keeps its 64 envs, probs tower only
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/goldsrl_gridtradenet.h"
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "flat_env_dev.h"

namespace grl {

enum : uint32_t { RS_GRIDTRADE_ACTION = 21 };    // next to RS_GRID_ACTION = 20 (net_discrete.hip)
constexpr int A3C_DPAD = 5;   // TradeAR1's processed observation with 2 assets, as in net_gauss.hip
constexpr bool A3C_PAD_LAST = true;
constexpr int GRID_D = 5;     // S0 = D = 5
constexpr int GRID_O = 2;     // outputs = assets
constexpr int GRID_KMAX = 48; // most grid points per output
constexpr uint32_t GRID_RS = RS_GRIDTRADE_ACTION;

#include "net_a3c_core.inc"
#include "net_a3c_grid.inc"

__global__ __launch_bounds__(256) void gt_forward_kernel(GridArgs a) {
    extern __shared__ float lds[];
    grid_forward(a, lds);
}

__global__ __launch_bounds__(256, 1) void gt_backward_kernel(GridArgs a) {
    extern __shared__ float lds[];
    grid_backward(a, lds);
}

#include "net_gridtrade_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"
#include "net_a3c_grid_host.h"

struct grl_gtnet : grl::GridNetBase {
    grl_gtnet_config cfg;
};

namespace grl {

struct GridTradeEnv {
    static constexpr auto forward = gt_forward_kernel, backward = gt_backward_kernel;
    static constexpr auto eval = gt_eval_kernel;
    static const float *obs(grl_handle *h) { return h->tr.obs; }
    static int step(grl_handle *h, const float *act, float *) { return trade_launch_step(h, act); }
    static int reset(grl_handle *h) { return trade_launch_reset(h, h->done_list, h->done_count, h->E); }
    static TradeParams params(grl_handle *h) { return trade_params(h); }
};

}  // namespace grl

using namespace grl;

extern "C" {

int grl_gtnet_config_default(grl_gtnet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_gtnet_config);
    cfg->rnn_length = 20; cfg->max_samples = 8192; cfg->lr_decay_steps = 100000; cfg->always_bootstrap = 0;
    cfg->num_choices = 17; cfg->num_outputs = GRID_O;
    cfg->scale = 1.f; cfg->gamma = 0.99f; cfg->gae_lambda = 0.96f; cfg->clip_norm = 40.f;
    cfg->rms_decay = 0.99f; cfg->rms_epsilon = 0.1f; cfg->lr_decay_rate = 0.96f;
    cfg->grid_lb = -1.0; cfg->grid_ub = 1.0;
    return GRL_OK;
}

int grl_gtnet_create(grl_handle *h, const grl_gtnet_config *cfg, grl_gtnet **out) {
    std::string msg;      // the refusals that carry numbers
    return a3c_create(
        "grl_gtnet_create", h, cfg, out,
        [&](const char *range) -> const char * {
            if (h->cfg.env_kind != GRL_ENV_TRADE) return "the grid trader needs a TradeAR1 handle";
            if (cfg->num_outputs != h->cfg.n_assets || h->cfg.n_assets != GRID_O) {
                msg = "num_outputs " + std::to_string(cfg->num_outputs) + " and the handle's " + std::to_string(h->cfg.n_assets) +
                      " assets: the device net has one output per asset and exists for " + std::to_string(GRID_O) + " assets";
                return msg.c_str();
            }
            if (range) return range;
            if (cfg->num_choices < 2 || cfg->num_choices > GRID_KMAX || !(cfg->grid_lb < cfg->grid_ub)) {
                msg = "num_choices " + std::to_string(cfg->num_choices) + ": 2.." + std::to_string(GRID_KMAX) + " (" + std::to_string(GRID_O) +
                      " outputs share the " + std::to_string(NX) + " logit rows), grid_lb < grid_ub";
                return msg.c_str();
            }
            if (cfg->always_bootstrap != 0) return "a TradeAR1 handle needs always_bootstrap = 0";
            // a symmetric grid with an odd number of points holds: its centre must be exactly 0.0f (goldsrl_gridtradenet.h)
            const int K = cfg->num_choices;
            if ((K & 1) && cfg->grid_lb == -cfg->grid_ub && grid_value((K - 1) / 2, K, cfg->grid_lb, cfg->grid_ub) != 0.0f)
                return "the centre of the symmetric grid does not come out as exactly 0: choose another num_choices";
            return nullptr;
        },
        [&](grl_gtnet *n, A3cGrow &Al) {
            n->S0 = n->D = GRID_D; n->K = cfg->num_choices;
            n->off = grid_offsets(n->K);
            const size_t ms = cfg->max_samples, E = h->E, OK = (size_t)GRID_O * n->K;
            n->ro_bufs = {a3c_buf("probs", &n->ro_probs, OK), a3c_buf("choices", &n->ro_choice, GRID_O), a3c_buf("actions", &n->ro_act, GRID_O)};
            n->ev_bufs = {a3c_buf("choices", &n->ev_choice, GRID_O), a3c_buf("actions", &n->ev_actions, GRID_O)};
            Al(&n->d_choice, ms * GRID_O); Al(&n->d_probs, ms * OK); Al(&n->ev_act, E * GRID_O);
            return (size_t)n->off.total;
        },
        {(const void *)gt_forward_kernel, (const void *)gt_backward_kernel, (const void *)gt_eval_kernel});
}

int grl_gtnet_destroy(grl_gtnet *n) { return a3c_destroy(n); }
const char *grl_gtnet_last_error(const grl_gtnet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_gtnet_num_params(const grl_gtnet *n) { return n ? n->num_params : 0; }
int grl_gtnet_set_params(grl_gtnet *n, const float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, (float *)host, cnt, true); }
int grl_gtnet_get_params(grl_gtnet *n, float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, host, cnt, false); }
int grl_gtnet_get_grads(grl_gtnet *n, int32_t which, float *host, int64_t cnt) { return a3c_get_grads(n, "grl_gtnet_get_grads", which, host, cnt); }
int grl_gtnet_get_optimizer_state(grl_gtnet *n, float *msp, float *msv, int64_t cnt, int64_t *step) { return a3c_get_optimizer_state(n, msp, msv, cnt, step); }
int grl_gtnet_set_optimizer_state(grl_gtnet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) { return a3c_set_optimizer_state(n, msp, msv, cnt, step); }
int grl_gtnet_get_action_counter(grl_gtnet *n, uint64_t *out) { return a3c_get_action_counter(n, out); }
int grl_gtnet_set_action_counter(grl_gtnet *n, uint64_t v) { return a3c_set_action_counter(n, v); }
int grl_gtnet_set_greedy(grl_gtnet *net, int32_t on) { return a3c_set_greedy(net, on); }

int grl_gtnet_predict(grl_gtnet *net, int32_t n, const float *states, const float *windows, float *probs, float *values) {
    return grid_predict<GridTradeEnv>(net, "grl_gtnet_predict", n, states, windows, probs, values);
}
int grl_gtnet_train(grl_gtnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                    const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    return grid_train<GridTradeEnv>(net, "grl_gtnet_train", n, states, windows, choices, adv, targets, weights, grad_mult, lr0, apply_update,
                                    stats_host);
}
int grl_gtnet_rollout(grl_gtnet *net, int32_t T) { return grid_rollout<GridTradeEnv>(net, "grl_gtnet_rollout", T); }
int grl_gtnet_eval(grl_gtnet *net, int32_t max_steps, int32_t trace_steps) { return grid_eval<GridTradeEnv>(net, "grl_gtnet_eval", max_steps, trace_steps); }
int grl_gtnet_read_eval(grl_gtnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_gtnet_read_eval", which, host, bytes); }
int grl_gtnet_train_rollout(grl_gtnet *net, float lr0, float *stats_host) {
    return grid_train_rollout<GridTradeEnv>(net, "grl_gtnet_train_rollout", lr0, stats_host);
}
int grl_gtnet_read_rollout(grl_gtnet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_gtnet_read_rollout", "", which, host, bytes);
}

}  // extern "C"
