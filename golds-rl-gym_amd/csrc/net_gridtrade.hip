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
//   teach    learning from the attainable optimum's table (include/goldsrl_gridtradeteach.h): second instantiations of the forward
//            (the teacher's look-up on waves 2 and 3, trade_dp_lookup.h) and of the backward (cross-entropy to its soft labels)
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/goldsrl_gridtradeteach.h"      // includes goldsrl_gridtradenet.h
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "flat_env_dev.h"
#include "trade_dp_lookup.h"

namespace grl {

enum : uint32_t { RS_GRIDTRADE_ACTION = 21 };    // next to RS_GRID_ACTION = 20 (net_discrete.hip)
enum : uint32_t { RS_GRIDTRADE_COIN = 22 };      // the teach rollout's coin: whose action steps the env (goldsrl_gridtradeteach.h)
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

// ---- the teacher (include/goldsrl_gridtradeteach.h): the attainable optimum's table on the handle, looked up on waves 2 and 3
// of the forward while waves 0 and 1 run the two heads.  What grid_forward<GtTeach> calls:
struct GtTeach {
    static constexpr bool on = true;
    TdpAxes A;
    const float *policy;                // the handle's table (horizon, [nu]^2, [nx]^2, 2)
    int horizon, max_steps, E;          // max_steps: the handle's TimeLimit, 0 without one
    const double *cash, *q, *p;         // the handle's raw account before the step; q, p (2,E)
    const int32_t *elapsed;
    double share;                       // agent_share
    float *act;                         // (E,O) the teacher's actions of this step
    int32_t *label_lo;                  // (E,O)
    float *label_w;                     // (E,O)

    // wave 2 + o, lane = env s: the statements of trade_dp_play_kernel (trade_dp_lookup.h) on the raw float64 account, then the
    // soft label of the float32 action on the net's own grid, float64, one IEEE operation per statement
    __device__ __forceinline__ float teacher(const GridArgs &a, int o, int s) const {
        const double qq[2] = {q[s], q[(size_t)E + s]}, pp[2] = {p[s], p[(size_t)E + s]};
        float ta[2];
        tdp_lookup<2>(A, policy, horizon, tdp_moves(max_steps, elapsed[s], horizon), cash[s], qq, pp, ta, o);
        const float t = o == 0 ? ta[0] : ta[1];
        const double step = (a.ub - a.lb) / (double)(a.K - 1);
        const double d = (double)t - a.lb;
        const double pos = d / step;
        int lo = (int)floor(pos);
        lo = lo < 0 ? 0 : (lo > a.K - 2 ? a.K - 2 : lo);
        const double r = pos - (double)lo;
        const size_t i = (size_t)s * GRID_O + o;
        act[i] = t; label_lo[i] = lo; label_w[i] = (float)fmin(fmax(r, 0.0), 1.0);
        return t;
    }
    // wave o, behind the barrier: the action env s is stepped with.  One uniform per (env, step), the first of the block of stream
    // RS_GRIDTRADE_COIN; agent_share 0 and 1 draw nothing.
    __device__ __forceinline__ float mix(const GridArgs &a, float own, float teach, int s) const {
        if (share <= 0.0) return teach;
        if (share < 1.0) {
            double u0, u1;
            u01_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GRIDTRADE_COIN, 0u), u0, u1);
            if (!(u0 < share)) return teach;
        }
        return own;
    }
};

__global__ __launch_bounds__(256) void gt_teach_forward_kernel(GridArgs a, GtTeach tt) {
    extern __shared__ float lds[];
    grid_forward(a, lds, tt);
}

__global__ __launch_bounds__(256, 1) void gt_teach_backward_kernel(GridArgs a, GridLabels tl) {
    extern __shared__ float lds[];
    grid_backward<true>(a, lds, tl);
}

#include "net_gridtrade_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"
#include "net_a3c_grid_host.h"

struct grl_gtnet : grl::GridNetBase {
    grl_gtnet_config cfg;
    // the teacher (goldsrl_gridtradeteach.h): its actions and labels per rollout step, the host-sample staging, the agreement sum
    float *ro_teach_act, *ro_label_w, *d_label_w;
    int32_t *ro_label_lo, *d_label_lo;
    double *teach_agree;
    bool ro_taught = false;                       // the last rollout was a teach rollout
    bool teach_ready = false;                     // the teach kernels' LDS limit is raised
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
            n->ro_bufs = {a3c_buf("probs", &n->ro_probs, OK), a3c_buf("choices", &n->ro_choice, GRID_O), a3c_buf("actions", &n->ro_act, GRID_O),
                          a3c_buf("teacher_actions", &n->ro_teach_act, GRID_O), a3c_buf("label_lo", &n->ro_label_lo, GRID_O),
                          a3c_buf("label_w", &n->ro_label_w, GRID_O)};
            n->ev_bufs = {a3c_buf("choices", &n->ev_choice, GRID_O), a3c_buf("actions", &n->ev_actions, GRID_O)};
            Al(&n->d_choice, ms * GRID_O); Al(&n->d_probs, ms * OK); Al(&n->ev_act, E * GRID_O);
            Al(&n->d_label_lo, ms * GRID_O); Al(&n->d_label_w, ms * GRID_O); Al(&n->teach_agree, 1);
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
int grl_gtnet_rollout(grl_gtnet *net, int32_t T) {
    if (net) net->ro_taught = false;
    return grid_rollout<GridTradeEnv>(net, "grl_gtnet_rollout", T);
}
int grl_gtnet_eval(grl_gtnet *net, int32_t max_steps, int32_t trace_steps) { return grid_eval<GridTradeEnv>(net, "grl_gtnet_eval", max_steps, trace_steps); }
int grl_gtnet_read_eval(grl_gtnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_gtnet_read_eval", which, host, bytes); }
int grl_gtnet_train_rollout(grl_gtnet *net, float lr0, float *stats_host) {
    return grid_train_rollout<GridTradeEnv>(net, "grl_gtnet_train_rollout", lr0, stats_host);
}
int grl_gtnet_read_rollout(grl_gtnet *net, const char *which, void *host, size_t bytes) {
    if (net && which && net->T && !net->ro_taught && (!strcmp(which, "teacher_actions") || !strcmp(which, "label_lo") || !strcmp(which, "label_w")))
        return a3c_fail(net, GRL_E_STATE, std::string("grl_gtnet_read_rollout: ") + which + " exists after grl_gtnet_teach_rollout; the last rollout was a plain one");
    return a3c_read_rollout(net, "grl_gtnet_read_rollout", "", which, host, bytes);
}

// ---- include/goldsrl_gridtradeteach.h

// the teach kernels' dynamic LDS limit, once per net
static int gt_teach_ready(grl_gtnet *net) {
    if (net->teach_ready) return GRL_OK;
    A3C_HIP(net, hipFuncSetAttribute((const void *)gt_teach_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)A3C_LDS));
    A3C_HIP(net, hipFuncSetAttribute((const void *)gt_teach_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)A3C_LDS));
    net->teach_ready = true;
    return GRL_OK;
}

// the supervised update over n device-resident samples: grid_train_device with the labels in place of choices and advantages
static int gt_teach_device(grl_gtnet *net, int n, const float *states, const float *win, const int32_t *lo, const float *w, const float *tgt,
                           const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = gt_teach_ready(net);
    if (rc || (rc = a3c_train_begin(net, n, a3c_scratch_trunk_rows(net->cfg.rnn_length), &blocks))) return rc;
    A3C_HIP(net, hipMemsetAsync(net->teach_agree, 0, sizeof(double), net->h->stream));
    GridArgs a = grid_args(net, n, states, win);
    a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    const GridLabels tl{lo, w, net->teach_agree};
    hipLaunchKernelGGL(gt_teach_backward_kernel, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a, tl);
    if ((rc = a3c_train_finish(net, blocks, net->off.p1w, (double)GRID_O, lr0, apply, stats_host))) return rc;      // synchronises
    if (stats_host) {      // the agreement: the weighted share of the (sample, output) pairs
        double agree, wsum;
        A3C_HIP(net, hipMemcpy(&agree, net->teach_agree, sizeof(double), hipMemcpyDeviceToHost));
        A3C_HIP(net, hipMemcpy(&wsum, net->stats64 + 3, sizeof(double), hipMemcpyDeviceToHost));
        stats_host[6] = wsum > 0.0 ? (float)(agree / ((double)GRID_O * wsum)) : 0.f;
    }
    return GRL_OK;
}

int grl_gtnet_teach_rollout(grl_gtnet *net, int32_t T, double agent_share) {
    const char *fn = "grl_gtnet_teach_rollout";
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": T >= 1");
    if (!(agent_share >= 0.0 && agent_share <= 1.0))
        return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": agent_share " + std::to_string(agent_share) + " is outside [0, 1]");
    grl_handle *h = net->h;
    const TradeDpState &d = h->tdp;
    if (d.horizon == 0)
        return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": the net's handle holds no table (grl_trade_dp_solve or grl_trade_dp_set_policy first)");
    hipSetDevice(h->cfg.device_id);
    int rc = gt_teach_ready(net);
    if (rc || (rc = a3c_ensure_rollout(net, T))) return rc;
    net->ro_taught = true;
    const size_t OK = (size_t)GRID_O * net->K;
    GtTeach tt{};
    tt.A = tdp_axes(d.grid, GRID_O); tt.policy = d.policy; tt.horizon = d.horizon; tt.max_steps = h->cfg.max_episode_steps; tt.E = h->E;
    tt.cash = h->tr.cash; tt.q = h->tr.q; tt.p = h->tr.p; tt.elapsed = h->elapsed; tt.share = agent_share;
    return a3c_rollout_run(
        net, T, GridTradeEnv::obs(h), [&](int n, const float *states, const float *win) { return grid_args(net, n, states, win); },
        [&](GridArgs &a, size_t o, int t) {
            a.probs = net->ro_probs + o * OK; a.act = net->ro_act + o * GRID_O; a.choice_out = net->ro_choice + o * GRID_O;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
            tt.act = net->ro_teach_act + o * GRID_O; tt.label_lo = net->ro_label_lo + o * GRID_O; tt.label_w = net->ro_label_w + o * GRID_O;
        },
        [&](const GridArgs &a) {
            if (!a.act) return grid_launch_fwd<GridTradeEnv>(net, a);      // the bootstrap pass: values only, no teacher
            hipLaunchKernelGGL(gt_teach_forward_kernel, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, h->stream, a, tt);
            A3C_HIP(net, hipGetLastError());
            return (int)GRL_OK;
        },
        [&](size_t o) { return GridTradeEnv::step(h, net->ro_act + o * GRID_O, net->term_obs); });
}

int grl_gtnet_train_teach_rollout(grl_gtnet *net, float lr0, float *stats_host) {
    const char *fn = "grl_gtnet_train_teach_rollout";
    if (net && net->T && !net->ro_taught) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": the last rollout was a plain one (grl_gtnet_teach_rollout first)");
    return a3c_train_rollout(net, fn, [&](int n, float mult) {
        return gt_teach_device(net, n, net->ro_states, net->ro_win, net->ro_label_lo, net->ro_label_w, net->ro_tgt, net->ro_wt, mult, lr0, 1, stats_host);
    });
}

int grl_gtnet_teach(grl_gtnet *net, int32_t n, const float *states, const float *windows, const int32_t *label_lo, const float *label_w,
                    const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    const char *fn = "grl_gtnet_teach";
    int rc = a3c_samples_check(net, fn, n, states && windows && label_lo && label_w && targets);
    if (rc) return rc;
    for (int64_t i = 0; i < (int64_t)n * GRID_O; ++i) {
        if (label_lo[i] < 0 || label_lo[i] > net->K - 2)
            return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": label_lo " + std::to_string(label_lo[i]) + " is outside [0, num_choices - 2] = [0, " +
                                                    std::to_string(net->K - 2) + "]");
        if (!(label_w[i] >= 0.f && label_w[i] <= 1.f))
            return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": label_w " + std::to_string(label_w[i]) + " is outside [0, 1]");
    }
    if ((rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_label_lo, label_lo, (size_t)n * GRID_O)) ||
        (rc = a3c_put(net, net->d_label_w, label_w, (size_t)n * GRID_O)) || (rc = a3c_stage_targets(net, n, nullptr, targets, weights)))
        return rc;
    return gt_teach_device(net, n, net->d_states, net->d_win, net->d_label_lo, net->d_label_w, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult, lr0,
                           apply_update, stats_host);
}

}  // extern "C"
