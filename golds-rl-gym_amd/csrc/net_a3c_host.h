// The host scaffold the A3C nets share (net_gated.hip, net_gauss.hip, net_discrete.hip): the state grl_gnet, grl_anet and grl_dnet
// derive from and one copy of what they do alike:
//   - the members all three own (parameters, optimizer, staging, rollout and bootstrap buffers, the evaluation's results and trace)
//   - one list per net of its rollout buffers and one of its evaluation buffers (A3cBuf: name, slot, bytes per row), from which
//     they are allocated (a3c_ensure_*) and read back by name (a3c_read_*): a width is written once, where the entry is made
//   - create (a3c_create), parameter / optimizer copies, the checks and staging copies of predict / train
//   - the training workspace and the update behind the backward kernel
//   - the rollout's steps (a3c_rollout_steps, on the widths' types) and the tail of the nets that bootstrap behind finished episodes
//   - the evaluation's checks, common arguments and closing reset
// Included behind net_a3c_core.inc (it launches its kernels); static: every including translation unit has its own copy.
// Functions take the C function's name where their message carries it.
#pragma once

namespace grl {

// A device buffer of the rollout or of the evaluation: rows of `row` bytes, one per step and env (T*E, S*E) or one per env.
// name: what read_rollout / read_eval know it by (null: not read back); present: false where the net's configuration keeps none.
struct A3cBuf {
    const char *name;
    void **slot;
    size_t row;
    bool per_env = false, present = true;
};
template <typename T>
static A3cBuf a3c_buf(const char *name, T **slot, size_t width, bool per_env = false, bool present = true) {
    return {name, (void **)slot, width * sizeof(T), per_env, present};
}

struct A3cNet {
    grl_handle *h = nullptr;
    std::string err;
    int64_t num_params = 0;
    float *params, *grads, *msp, *msv, *stats;    // grads: [policy P | value P]
    double *stats64;                              // 4 loss sums, then 2 x kA3cSumsqBlocks partial sums
    int64_t global_step = 0;
    uint64_t act_counter = 0;
    int greedy = 0;                               // grl_*net_set_greedy
    int S0 = 0, D = 0, toff = 0;                  // processed observation, temporal row and where in the observation it starts
    // host-sample staging
    float *d_states, *d_win, *d_adv, *d_tgt, *d_wt, *d_vals;
    // training workspace (grown on demand)
    float *slab, *scratch;
    int ws_blocks = 0;
    // rollout
    float *win;                                   // (E,R,D) each env's current window
    int32_t *kstep;
    int win_init = 0;
    int T = 0;
    float *ro_states, *ro_win, *ro_val, *ro_rew, *ro_done, *ro_mask, *ro_wt, *ro_adv, *ro_tgt, *ro_boot, *boot_states, *boot_win;
    // grl_*net_eval: per-env results, the trace of the first ev_trace steps
    double *ev_total;
    int32_t *ev_len;
    uint8_t *ev_fin;
    float *ev_states, *ev_actions, *ev_rew, *ev_done;
    int32_t ev_reset_count;                       // E, the source of the reset list's count (outlives the async copy)
    int ev_trace = 0, ev_trace_cap = -1, ev_played = -2;      // ev_played: -1 until read_eval has looked, -2 before any evaluation
    std::vector<void *> allocs, ro_allocs, ws_allocs, ev_allocs;
    std::vector<A3cBuf> ro_bufs, ev_bufs;         // every rollout / evaluation buffer: the shared ones, then the net's heads'
};

static int a3c_fail(A3cNet *n, int code, const std::string &msg) {
    if (n) n->err = msg;
    return code;
}
#define A3C_HIP(n, call)                                                                                      \
    do {                                                                                                      \
        hipError_t _e = (call);                                                                               \
        if (_e != hipSuccess) return a3c_fail(n, GRL_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
static int a3c_alloc(A3cNet *n, T **p, size_t count, std::vector<void *> &list) {
    A3C_HIP(n, hipMalloc((void **)p, (count ? count : 1) * sizeof(T)));
    list.push_back(*p);
    A3C_HIP(n, hipMemsetAsync(*p, 0, (count ? count : 1) * sizeof(T), n->h->stream));
    return GRL_OK;
}

// a run of allocations into one list that stops at the first failure
struct A3cGrow {
    A3cNet *n;
    std::vector<void *> &list;
    int rc = GRL_OK;
    template <typename T>
    void operator()(T **p, size_t count) { if (rc == GRL_OK) rc = a3c_alloc(n, p, count, list); }
};

// wait for the stream and free a list's buffers: the first half of growing them
static int a3c_release(A3cNet *n, std::vector<void *> &list) {
    A3C_HIP(n, hipStreamSynchronize(n->h->stream));
    for (void *p : list) hipFree(p);
    list.clear();
    return GRL_OK;
}

// allocate a list's per-env buffers (at creation) or its per-step buffers for `rows` rows
static int a3c_alloc_bufs(A3cNet *n, std::vector<A3cBuf> &bufs, bool per_env, size_t rows, std::vector<void *> &list) {
    A3cGrow Al{n, list};
    for (A3cBuf &b : bufs) {
        if (b.per_env != per_env) continue;
        *b.slot = nullptr;
        if (b.present) Al((char **)b.slot, rows * b.row);
    }
    return Al.rc;
}

// grow a list's per-step buffers on demand: release, allocate for `steps` steps, record the capacity (`unset` while there is none)
static int a3c_ensure(A3cNet *n, std::vector<A3cBuf> &bufs, std::vector<void *> &list, int &cap, int unset, int steps) {
    int rc = a3c_release(n, list);
    if (rc) return rc;
    cap = unset;
    if ((rc = a3c_alloc_bufs(n, bufs, false, (size_t)steps * n->h->E, list)) == GRL_OK) cap = steps;
    return rc;
}
static int a3c_ensure_rollout(A3cNet *n, int T) { return T == n->T ? GRL_OK : a3c_ensure(n, n->ro_bufs, n->ro_allocs, n->T, 0, T); }
// the trace only grows
static int a3c_ensure_trace(A3cNet *n, int steps) {
    return steps <= n->ev_trace_cap ? GRL_OK : a3c_ensure(n, n->ev_bufs, n->ev_allocs, n->ev_trace_cap, -1, steps);
}

// what every net owns at creation, from its widths S0 / D (set before) and R = rnn_length, ms = max_samples: the shared entries
// of both buffer lists (the net's own are there already), everything that exists from creation on, then the RMSProp ms at ones (TF 1.x)
static int a3c_create_common(A3cNet *n, size_t P, size_t E, size_t R, size_t ms) {
    n->num_params = (int64_t)P;
    const size_t S0 = n->S0, W = R * n->D;
    n->ro_bufs.insert(n->ro_bufs.end(),
                      {a3c_buf("states", &n->ro_states, S0), a3c_buf("windows", &n->ro_win, W), a3c_buf("values", &n->ro_val, 1),
                       a3c_buf("rewards", &n->ro_rew, 1), a3c_buf("dones", &n->ro_done, 1), a3c_buf(nullptr, &n->ro_mask, 1),
                       a3c_buf("weights", &n->ro_wt, 1), a3c_buf("adv", &n->ro_adv, 1), a3c_buf("targets", &n->ro_tgt, 1),
                       a3c_buf("boot", &n->ro_boot, 1, true)});
    n->ev_bufs.insert(n->ev_bufs.end(),
                      {a3c_buf("total_reward", &n->ev_total, 1, true), a3c_buf("length", &n->ev_len, 1, true),
                       a3c_buf("finished", &n->ev_fin, 1, true), a3c_buf("states", &n->ev_states, S0), a3c_buf("rewards", &n->ev_rew, 1),
                       a3c_buf("dones", &n->ev_done, 1)});
    A3cGrow Al{n, n->allocs};
    Al(&n->params, P); Al(&n->grads, 2 * P); Al(&n->msp, P); Al(&n->msv, P); Al(&n->stats, 8);
    Al(&n->stats64, 4 + 2 * kA3cSumsqBlocks); Al(&n->kstep, E);
    Al(&n->d_states, ms * S0); Al(&n->d_win, ms * W); Al(&n->d_adv, ms); Al(&n->d_tgt, ms); Al(&n->d_wt, ms); Al(&n->d_vals, ms);
    Al(&n->win, E * W); Al(&n->boot_states, E * S0); Al(&n->boot_win, E * W);
    if (Al.rc == GRL_OK) Al.rc = a3c_alloc_bufs(n, n->ro_bufs, true, E, n->allocs);
    if (Al.rc == GRL_OK) Al.rc = a3c_alloc_bufs(n, n->ev_bufs, true, E, n->allocs);
    if (Al.rc != GRL_OK) return Al.rc;
    hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, n->h->stream, n->msp, (long)P, 1.0f);
    hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, n->h->stream, n->msv, (long)P, 1.0f);
    A3C_HIP(n, hipGetLastError());
    return GRL_OK;
}

template <typename NET>
static int a3c_destroy(NET *n) {
    if (!n) return GRL_OK;
    grl_sync_for_destroy(n->h);
    for (auto *list : {&n->allocs, &n->ro_allocs, &n->ws_allocs, &n->ev_allocs})
        for (void *p : *list) hipFree(p);
    delete n;
    return GRL_OK;
}

static int a3c_copy(A3cNet *n, float *dev, float *host, int64_t cnt, bool to_dev) {
    if (!n || !host) return a3c_fail(n, GRL_E_INVALID, "null argument");
    if (cnt != n->num_params) return a3c_fail(n, GRL_E_SIZE, "length must be num_params");
    hipSetDevice(n->h->cfg.device_id);
    A3C_HIP(n, hipStreamSynchronize(n->h->stream));
    A3C_HIP(n, hipMemcpy(to_dev ? (void *)dev : (void *)host, to_dev ? (const void *)host : (const void *)dev, (size_t)cnt * 4,
                         to_dev ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return GRL_OK;
}

static int a3c_get_grads(A3cNet *n, const char *fn, int32_t which, float *host, int64_t cnt) {
    if (n && which != 0 && which != 1) return a3c_fail(n, GRL_E_INVALID, std::string(fn) + ": which is 0 or 1");
    return a3c_copy(n, n ? n->grads + (which ? n->num_params : 0) : nullptr, host, cnt, false);
}

static int a3c_get_optimizer_state(A3cNet *n, float *msp, float *msv, int64_t cnt, int64_t *step) {
    int rc = a3c_copy(n, n ? n->msp : nullptr, msp, cnt, false);
    if (!rc) rc = a3c_copy(n, n->msv, msv, cnt, false);
    if (!rc && step) *step = n->global_step;
    return rc;
}

static int a3c_set_optimizer_state(A3cNet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) {
    if (n && step < 0) return a3c_fail(n, GRL_E_INVALID, "global step must be >= 0");
    int rc = a3c_copy(n, n ? n->msp : nullptr, (float *)msp, cnt, true);
    if (!rc) rc = a3c_copy(n, n->msv, (float *)msv, cnt, true);
    if (!rc) n->global_step = step;
    return rc;
}

static int a3c_get_action_counter(A3cNet *n, uint64_t *out) {
    if (!n || !out) return GRL_E_INVALID;
    *out = n->act_counter;
    return GRL_OK;
}

static int a3c_set_action_counter(A3cNet *n, uint64_t v) {
    if (!n) return GRL_E_INVALID;
    n->act_counter = v;
    return GRL_OK;
}

static int a3c_set_greedy(A3cNet *n, int32_t on) {
    if (!n) return GRL_E_INVALID;
    n->greedy = on ? 1 : 0;
    return GRL_OK;
}

// grl_*net_create under its name fn.  The net brings
//   env_check(range)   its refusals as a message without the name, or null: the handle's env kind, then `range` (the message of
//                      the range check all three share, null if the config passed), then what the net itself bounds
//   setup(n, Al)       the widths S0 / D / toff, the offsets, the net's own entries of both buffer lists and, through Al, the
//                      buffers only it has; returns the number of parameters
//   kernels            the three whose dynamic LDS limit is raised
template <typename NET, typename CFG, typename CHECK, typename SETUP>
static int a3c_create(const char *fn, grl_handle *h, const CFG *cfg, NET **out, CHECK env_check, SETUP setup, const void *const (&kernels)[3]) {
    if (!h || !cfg || !out) return GRL_E_INVALID;
    *out = nullptr;
    const std::string name = std::string(fn) + ": ";
    if (cfg->struct_size != (int32_t)sizeof(CFG)) return fail(h, GRL_E_INVALID, name + "config size mismatch");
    const bool in_range = cfg->rnn_length >= 1 && cfg->rnn_length <= MAXR && cfg->max_samples >= 1 && cfg->lr_decay_steps >= 1 &&
                          cfg->scale != 0.f && cfg->gae_lambda > 0.f && cfg->gae_lambda <= 1.f;
    if (const char *msg = env_check(in_range ? nullptr : "config out of range (rnn_length 1..20)")) return fail(h, GRL_E_INVALID, name + msg);
    hipSetDevice(h->cfg.device_id);
    NET *n = new NET();
    n->h = h; n->cfg = *cfg;
    A3cGrow Al{n, n->allocs};
    const size_t P = setup(n, Al);
    int rc = Al.rc;
    if (rc == GRL_OK) rc = a3c_create_common(n, P, h->E, cfg->rnn_length, cfg->max_samples);
    if (rc == GRL_OK) {
        hipError_t e = hipGetLastError();
        for (const void *k : kernels)
            if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)A3C_LDS);
        if (e != hipSuccess) rc = a3c_fail(n, GRL_E_HIP, name + hipGetErrorString(e));
    }
    if (rc != GRL_OK) {
        fail(h, rc, name + n->err);
        a3c_destroy(n);
        return rc;
    }
    hipStreamSynchronize(h->stream);
    *out = n;
    return GRL_OK;
}

// predict / train on host samples: the argument checks (ok: the call's pointers are there) ...
template <typename NET>
static int a3c_samples_check(NET *net, const char *fn, int n, bool ok) {
    if (!net || n <= 0 || !ok) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": bad argument");
    if (n > net->cfg.max_samples) return a3c_fail(net, GRL_E_SIZE, std::string(fn) + ": n exceeds max_samples");
    return GRL_OK;
}
// ... and count elements to or from a staging buffer on the net's stream (a null source or destination: nothing to copy)
template <typename T>
static int a3c_put(A3cNet *net, T *dev, const T *host, size_t count) {
    if (host) A3C_HIP(net, hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, net->h->stream));
    return GRL_OK;
}
template <typename T>
static int a3c_get(A3cNet *net, T *host, const T *dev, size_t count) {
    if (host) A3C_HIP(net, hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return GRL_OK;
}
// the n samples' states and windows into d_states / d_win
template <typename NET>
static int a3c_stage(NET *net, int n, const float *states, const float *windows) {
    hipSetDevice(net->h->cfg.device_id);
    int rc = a3c_put(net, net->d_states, states, (size_t)n * net->S0);
    return rc ? rc : a3c_put(net, net->d_win, windows, (size_t)n * net->cfg.rnn_length * net->D);
}
// train's advantages, targets and, if given, weights into d_adv / d_tgt / d_wt
static int a3c_stage_targets(A3cNet *net, int n, const float *adv, const float *targets, const float *weights) {
    int rc = a3c_put(net, net->d_adv, adv, n);
    if (!rc) rc = a3c_put(net, net->d_tgt, targets, n);
    return rc ? rc : a3c_put(net, net->d_wt, weights, n);
}

// before the backward kernel: its slabs and scratch for the workgroups of n samples (grown on demand), cleared slabs and loss sums
static int a3c_train_begin(A3cNet *net, int n, int scratch_rows, int *blocks_out) {
    const int groups = (n + 63) / 64, blocks = groups < 256 ? groups : 256;      // 154 KB of LDS: one workgroup per CU
    const size_t P = (size_t)net->num_params;
    if (blocks > net->ws_blocks) {
        int rc = a3c_release(net, net->ws_allocs);
        if (rc) return rc;
        net->ws_blocks = 0;
        A3cGrow Al{net, net->ws_allocs};
        Al(&net->slab, (size_t)blocks * 2 * P); Al(&net->scratch, (size_t)blocks * scratch_rows * 64);
        if (Al.rc) return Al.rc;
        net->ws_blocks = blocks;
    }
    A3C_HIP(net, hipMemsetAsync(net->slab, 0, (size_t)blocks * 2 * P * sizeof(float), net->h->stream));
    A3C_HIP(net, hipMemsetAsync(net->stats64, 0, 4 * sizeof(double), net->h->stream));
    *blocks_out = blocks;
    return GRL_OK;
}

// behind the backward kernel: the slabs' sum in a fixed order, norms, clip factors and (apply) both RMSProp steps.  first_tower =
// the offset where the trunk ends, heads = the entropy terms per sample.
template <typename NET>
static int a3c_train_finish(NET *net, int blocks, long first_tower, double heads, float lr0, int apply, float *stats_host) {
    hipStream_t st = net->h->stream;
    const long P = net->off.total;
    hipLaunchKernelGGL(flat_slab_reduce_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(1024), 0, st, net->slab, blocks, 2 * P, net->grads);
    hipLaunchKernelGGL(a3c_sumsq_kernel, dim3(kA3cSumsqBlocks, 2), dim3(256), 0, st, net->grads, P, net->stats64 + 4);
    // tf.train.exponential_decay(lr0, global_step, decay_steps, rate, staircase=False), global_step before the update
    const float lr = (float)((double)lr0 * pow((double)net->cfg.lr_decay_rate, (double)net->global_step / (double)net->cfg.lr_decay_steps));
    hipLaunchKernelGGL(a3c_finalize_kernel, dim3(1), dim3(64), 0, st, net->stats64, net->stats64 + 4, heads, net->cfg.clip_norm, lr, net->stats);
    if (apply) {
        hipLaunchKernelGGL(a3c_rmsprop_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, net->params, net->grads, net->msp, net->msv, P,
                           first_tower, net->off.v1w, net->stats, net->cfg.rms_decay, net->cfg.rms_epsilon);
        net->global_step += 2;      // both train ops increment it (estimators.py:137-140 / 325-328, 403-406 / 409-412)
    }
    A3C_HIP(net, hipGetLastError());
    A3C_HIP(net, hipStreamSynchronize(st));
    if (stats_host) {
        float s[6];
        A3C_HIP(net, hipMemcpy(s, net->stats, sizeof(s), hipMemcpyDeviceToHost));
        for (int i = 0; i < 6; ++i) stats_host[i] = s[i];
    }
    return GRL_OK;
}

// The steps of a rollout on the widths S0 / D / toff as types (ints at run time, or integral constants): the windows brought up to
// the handle's episodes, T steps of record, forward + action, env step, episode accounting and window rule, then V of the window
// after the last step into ro_boot.  term_obs / term_st / term_wn: where the env leaves and the rollout keeps the observation and
// window behind a finished episode, or null.  The net brings what differs:
//   args(n, states, windows)   its forward's argument block (field vals is set here)
//   acting(a, o, t)            the heads' outputs and the action of step t into the rollout buffers at sample offset o = t * E
//   fwd(a)                     the forward launch
//   env_step(o)                the env's step on the actions recorded at o
template <typename S0T, typename DT, typename TOFFT, typename ARGS, typename ACTING, typename FWD, typename STEP>
static int a3c_rollout_steps(A3cNet *net, int T, int R, const float *obs, S0T S0, DT D, TOFFT toff, const float *term_obs, float *term_st,
                             float *term_wn, ARGS args, ACTING acting, FWD fwd, STEP env_step) {
    grl_handle *h = net->h;
    hipStream_t st = h->stream;
    const int E = h->E, eb = (E + 255) / 256;
    const size_t s0 = net->S0, w = (size_t)R * net->D;
    float *const none = nullptr;
    int rc;
    hipLaunchKernelGGL((a3c_sync_kernel<S0T, DT, TOFFT>), dim3(eb), dim3(256), 0, st, h->elapsed, obs, net->win, net->kstep, E, R, S0, D, toff,
                       net->win_init ? 0 : 1);
    net->win_init = 1;
    for (int t = 0; t < T; ++t) {
        const size_t o = (size_t)t * E;
        hipLaunchKernelGGL((a3c_record_kernel<S0T, DT>), dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, S0, D, net->ro_states + o * s0,
                           net->ro_win + o * w, net->ro_wt + o);
        auto a = args(E, net->ro_states + o * s0, net->ro_win + o * w);
        a.vals = net->ro_val + o;
        acting(a, o, t);
        if ((rc = fwd(a))) return rc;
        if ((rc = env_step(o))) return a3c_fail(net, rc, h->err);
        if ((rc = episodes_launch_account(h))) return a3c_fail(net, rc, h->err);
        hipLaunchKernelGGL((a3c_post_kernel<S0T, DT, TOFFT>), dim3(eb), dim3(256), 0, st, h->reward, h->done, obs, term_obs, net->win, net->kstep, E, R,
                           S0, D, toff, net->ro_rew + o, net->ro_done + o, net->ro_mask + o, term_st ? term_st + o * s0 : none,
                           term_wn ? term_wn + o * w : none);
    }
    if (!net->greedy) net->act_counter += (uint64_t)T;      // a greedy rollout draws nothing
    hipLaunchKernelGGL((a3c_record_kernel<S0T, DT>), dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, S0, D, net->boot_states, net->boot_win,
                       none);
    auto b = args(E, net->boot_states, net->boot_win);
    b.vals = net->ro_boot;
    return fwd(b);
}

// The rollout of the nets whose temporal row is the whole processed observation (the Gaussian and the discrete agent; obs = the
// handle's processed observation): the steps; then, with always_bootstrap, V behind every finished episode (field gate: workgroups
// whose 64 samples ended none leave at once), and the worker's GAE (worker.py:241-294).  The net has ro_term_st, ro_term_wn,
// ro_term_val and term_obs by these names.
template <typename NET, typename ARGS, typename ACTING, typename FWD, typename STEP>
static int a3c_rollout_run(NET *net, int T, const float *obs, ARGS args, ACTING acting, FWD fwd, STEP env_step) {
    hipStream_t st = net->h->stream;
    const int E = net->h->E, ab = net->cfg.always_bootstrap;
    const size_t TE = (size_t)T * E;
    if (ab) A3C_HIP(net, hipMemsetAsync(net->ro_term_val, 0, TE * sizeof(float), st));      // steps that end no episode read 0
    int rc = a3c_rollout_steps(net, T, net->cfg.rnn_length, obs, net->D, net->D, 0, ab ? net->term_obs : (const float *)nullptr, net->ro_term_st,
                               net->ro_term_wn, args, acting, fwd, env_step);
    if (rc) return rc;
    if (ab) {
        auto c = args((int)TE, net->ro_term_st, net->ro_term_wn);
        c.gate = net->ro_done; c.vals = net->ro_term_val;
        if ((rc = fwd(c))) return rc;
    }
    hipLaunchKernelGGL(a3c_returns_kernel<float>, dim3((E + 255) / 256), dim3(256), 0, st, net->ro_rew, net->ro_val, net->ro_done, net->ro_term_val,
                       net->ro_boot, T, E, net->cfg.gamma, net->cfg.gae_lambda, net->cfg.scale, ab, net->ro_tgt, net->ro_adv);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// grl_*net_train_rollout: the guards; train(n, mult) is the net's update on the T * E recorded samples, each gradient over E
template <typename TRAIN>
static int a3c_train_rollout(A3cNet *net, const char *fn, TRAIN train) {
    if (!net) return GRL_E_INVALID;
    if (!net->T) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    const int E = net->h->E;
    return train(net->T * E, 1.0f / (float)E);
}

// grl_*net_eval before its launch: the argument checks, the net's own guards, the trace buffers for min(trace_steps, max_steps) steps
template <typename GUARD>
static int a3c_eval_begin(A3cNet *net, const char *fn, int32_t max_steps, int32_t *trace_steps, GUARD guard) {
    if (!net) return GRL_E_INVALID;
    if (max_steps < 1 || *trace_steps < 0) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": max_steps >= 1, trace_steps >= 0");
    hipSetDevice(net->h->cfg.device_id);
    int rc = guard();
    if (rc) return rc;
    if (*trace_steps > max_steps) *trace_steps = max_steps;
    return a3c_ensure_trace(net, *trace_steps);
}
static int a3c_eval_begin(A3cNet *net, const char *fn, int32_t max_steps, int32_t *trace_steps) {
    return a3c_eval_begin(net, fn, max_steps, trace_steps, [] { return GRL_OK; });
}

// the fields every net's evaluation arguments name alike
template <typename EV>
static void a3c_eval_args(A3cNet *net, EV &v, int max_steps, int trace_steps) {
    v.win = net->win; v.max_steps = max_steps; v.trace_steps = trace_steps;
    v.total = net->ev_total; v.length = net->ev_len; v.finished = net->ev_fin;
    v.tr_states = net->ev_states; v.tr_rew = net->ev_rew; v.tr_done = net->ev_done;
}

// behind the evaluation kernel: the list and count of the handle's full reset, as grl_reset(h, NULL, 0) enqueues them, then the
// env's reset on h->done_list / h->done_count (reset())
template <typename RESET>
static int a3c_eval_finish(A3cNet *net, int trace_steps, RESET reset) {
    grl_handle *h = net->h;
    A3C_HIP(net, hipGetLastError());
    net->ev_trace = trace_steps;
    net->ev_played = -1;
    net->win_init = 0;      // the windows were the evaluation's: the next rollout starts every env's anew
    int rc = launch_iota(h, h->done_list, h->E);
    if (rc) return a3c_fail(net, rc, h->err);
    net->ev_reset_count = h->E;
    A3C_HIP(net, hipMemcpyAsync(h->done_count, &net->ev_reset_count, 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = reset())) return a3c_fail(net, rc, h->err);
    return GRL_OK;
}

// rows of the evaluation's trace that hold something: E x min(trace steps, steps the call played = the longest episode)
static int a3c_eval_rows(A3cNet *net, const char *fn, size_t *rows) {
    if (net->ev_played == -2) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": no evaluation yet");
    hipSetDevice(net->h->cfg.device_id);
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t E = net->h->E;
    if (net->ev_played < 0) {
        std::vector<int32_t> len(E);
        A3C_HIP(net, hipMemcpy(len.data(), net->ev_len, E * 4, hipMemcpyDeviceToHost));
        int32_t mx = 0;
        for (int32_t l : len) mx = l > mx ? l : mx;
        net->ev_played = mx;
    }
    *rows = (size_t)(net->ev_trace < net->ev_played ? net->ev_trace : net->ev_played) * E;
    return GRL_OK;
}

// a buffer of a list by name, `rows` rows of its per-step entries; absent: what to say of one the net's configuration does not keep
static int a3c_read(A3cNet *net, const char *fn, const std::vector<A3cBuf> &bufs, size_t rows, const char *absent, const char *which, void *host,
                    size_t bytes) {
    const A3cBuf *e = nullptr;
    for (const A3cBuf &b : bufs)
        if (b.name && !strcmp(which, b.name)) e = &b;
    if (e && !e->present) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": " + which + absent);
    if (!e) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": unknown buffer " + which);
    if (bytes != (e->per_env ? net->h->E : rows) * e->row) return a3c_fail(net, GRL_E_SIZE, std::string(fn) + ": wrong size for " + which);
    hipSetDevice(net->h->cfg.device_id);
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if (bytes) A3C_HIP(net, hipMemcpy(host, *e->slot, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

static int a3c_read_rollout(A3cNet *net, const char *fn, const char *absent, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": bad argument");
    if (!net->T) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": no rollout yet");
    return a3c_read(net, fn, net->ro_bufs, (size_t)net->T * net->h->E, absent, which, host, bytes);
}

static int a3c_read_eval(A3cNet *net, const char *fn, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": bad argument");
    size_t rows;
    int rc = a3c_eval_rows(net, fn, &rows);
    return rc ? rc : a3c_read(net, fn, net->ev_bufs, rows, "", which, host, bytes);
}

}  // namespace grl
