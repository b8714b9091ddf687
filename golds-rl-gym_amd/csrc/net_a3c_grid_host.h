// The host half the two softmax-grid nets share (net_discrete.hip, net_gridtrade.hip), behind net_a3c_grid.inc's device half:
// the members both own for the head and one copy of the calls they make alike.  Included behind net_a3c_host.h; static: each
// including translation unit has its own copy, on its own GRID_D / GRID_O.  A net derives from GridNetBase, adds its config as
// `cfg`, keeps its own create (refusals and buffer lists) and describes its env and kernels in a struct ENV:
//   forward, backward, eval     the net's three kernels
//   obs(h)                      the handle's processed observation (E,D)
//   step(h, act, term_obs)      the env's step launch on (E,O) actions; term_obs: where a handle that bootstraps behind finished
//                               episodes leaves their last observation (null where the net has no terminal-pass buffers)
//   reset(h)                    the env's reset launch on h->done_list / h->done_count
//   params(h)                   what the evaluation kernel takes to step the env
// Functions take the C function's name where their message carries it.
#pragma once

namespace grl {

struct GridNetBase : A3cNet {
    GridOff off;
    int K;                                        // grid points per output; S0 = D = GRID_D, the processed observation
    // the head's host-sample staging, rollout buffers and evaluation trace
    float *d_probs;
    int32_t *d_choice;
    float *ro_probs, *ro_act;                     // ro_act (T,E,O): the grid values each env was stepped with
    int32_t *ro_choice;
    // the rollout loop's terminal-pass buffers: only a net whose handle needs always_bootstrap = 1 allocates them
    float *ro_term_st = nullptr, *ro_term_wn = nullptr, *ro_term_val = nullptr, *term_obs = nullptr;
    float *ev_act;                                // (E,O): the evaluation step's actions
    int32_t *ev_choice;
};

template <typename NET>
static GridArgs grid_args(NET *net, int n, const float *states, const float *win) {
    GridArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.K = net->K; a.scale = net->cfg.scale;
    a.lb = net->cfg.grid_lb; a.ub = net->cfg.grid_ub;
    a.states = states; a.win = win; a.mult = 1.0f;
    return a;
}

template <typename ENV, typename NET>
static int grid_launch_fwd(NET *net, const GridArgs &a) {
    hipLaunchKernelGGL(ENV::forward, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
template <typename ENV, typename NET>
static int grid_train_device(NET *net, int n, const float *states, const float *win, const int32_t *choice, const float *adv, const float *tgt,
                             const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = a3c_train_begin(net, n, a3c_scratch_trunk_rows(net->cfg.rnn_length), &blocks);
    if (rc) return rc;
    GridArgs a = grid_args(net, n, states, win);
    a.choice = choice; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    hipLaunchKernelGGL(ENV::backward, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    return a3c_train_finish(net, blocks, net->off.p1w, (double)GRID_O, lr0, apply, stats_host);
}

template <typename ENV, typename NET>
static int grid_predict(NET *net, const char *fn, int32_t n, const float *states, const float *windows, float *probs, float *values) {
    int rc = a3c_samples_check(net, fn, n, states && windows);
    if (rc || (rc = a3c_stage(net, n, states, windows))) return rc;
    GridArgs a = grid_args(net, n, net->d_states, net->d_win);
    a.probs = net->d_probs; a.vals = net->d_vals;
    if ((rc = grid_launch_fwd<ENV>(net, a))) return rc;
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if ((rc = a3c_get(net, probs, net->d_probs, (size_t)n * GRID_O * net->K))) return rc;
    return a3c_get(net, values, net->d_vals, n);
}

template <typename ENV, typename NET>
static int grid_train(NET *net, const char *fn, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                      const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    int rc = a3c_samples_check(net, fn, n, states && windows && choices && adv && targets);
    if (rc) return rc;
    for (int64_t i = 0; i < (int64_t)n * GRID_O; ++i)
        if (choices[i] < 0 || choices[i] >= net->K) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": a choice outside [0, num_choices)");
    if ((rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_choice, choices, (size_t)n * GRID_O)) ||
        (rc = a3c_stage_targets(net, n, adv, targets, weights)))
        return rc;
    return grid_train_device<ENV>(net, n, net->d_states, net->d_win, net->d_choice, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult,
                                  lr0, apply_update, stats_host);
}

template <typename ENV, typename NET>
static int grid_rollout(NET *net, const char *fn, int32_t T) {
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = a3c_ensure_rollout(net, T);
    if (rc) return rc;
    const size_t OK = (size_t)GRID_O * net->K;
    return a3c_rollout_run(
        net, T, ENV::obs(h), [&](int n, const float *states, const float *win) { return grid_args(net, n, states, win); },
        [&](GridArgs &a, size_t o, int t) {
            a.probs = net->ro_probs + o * OK; a.act = net->ro_act + o * GRID_O; a.choice_out = net->ro_choice + o * GRID_O;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
        },
        [&](const GridArgs &a) { return grid_launch_fwd<ENV>(net, a); },
        [&](size_t o) { return ENV::step(h, net->ro_act + o * GRID_O, net->term_obs); });
}

template <typename ENV, typename NET>
static int grid_eval(NET *net, const char *fn, int32_t max_steps, int32_t trace_steps) {
    int rc = a3c_eval_begin(net, fn, max_steps, &trace_steps);
    if (rc) return rc;
    grl_handle *h = net->h;
    const int E = h->E;
    GridEvalArgs v{};
    v.a = grid_args(net, E, ENV::obs(h), net->win);
    a3c_eval_args(net, v, max_steps, trace_steps);
    v.act = net->ev_act; v.tr_choice = net->ev_choice; v.tr_act = net->ev_actions;
    hipLaunchKernelGGL(ENV::eval, dim3((E + 63) / 64), dim3(256), A3C_LDS, h->stream, v, ENV::params(h));
    return a3c_eval_finish(net, trace_steps, [&] { return ENV::reset(h); });
}

template <typename ENV, typename NET>
static int grid_train_rollout(NET *net, const char *fn, float lr0, float *stats_host) {
    return a3c_train_rollout(net, fn, [&](int n, float mult) {
        return grid_train_device<ENV>(net, n, net->ro_states, net->ro_win, net->ro_choice, net->ro_adv, net->ro_tgt, net->ro_wt, mult, lr0, 1,
                                      stats_host);
    });
}

}  // namespace grl
