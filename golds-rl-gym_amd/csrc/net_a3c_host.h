// The host scaffold the A3C nets share (net_gated.hip, net_gauss.hip, net_discrete.hip): the state grl_gnet, grl_anet and grl_dnet
// derive from and one copy of what they do alike -- allocation lists, parameter / optimizer copies, the training workspace, the update behind the backward
// kernel, the evaluation's closing reset and the named read-backs.  Included behind net_a3c_core.inc (it launches its kernels);
// static: every including translation unit has its own copy.  Functions take the C function's name where their message carries it.
#pragma once

namespace grl {

struct A3cNet {
    grl_handle *h = nullptr;
    std::string err;
    int64_t num_params = 0;
    float *params, *grads, *msp, *msv, *stats;    // grads: [policy P | value P]
    double *stats64;                              // 4 loss sums, then 2 x kA3cSumsqBlocks partial sums
    int64_t global_step = 0;
    uint64_t act_counter = 0;
    int greedy = 0;                               // grl_*net_set_greedy
    // training workspace (grown on demand)
    float *slab, *scratch;
    int ws_blocks = 0;
    // rollout
    float *win;                                   // (E,R,D) each env's current window
    int32_t *kstep;
    int win_init = 0;
    int T = 0;
    // grl_*net_eval: per-env results
    double *ev_total;
    int32_t *ev_len;
    uint8_t *ev_fin;
    int32_t ev_reset_count;                       // E, the source of the reset list's count (outlives the async copy)
    int ev_trace = 0, ev_trace_cap = -1, ev_played = -2;      // ev_played: -1 until read_eval has looked, -2 before any evaluation
    std::vector<void *> allocs, ro_allocs, ws_allocs, ev_allocs;
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

// what every net owns at creation, then the RMSProp ms at ones (TF 1.x)
static int a3c_create_common(A3cNet *n, size_t P, size_t E) {
    n->num_params = (int64_t)P;
    A3cGrow Al{n, n->allocs};
    Al(&n->params, P); Al(&n->grads, 2 * P); Al(&n->msp, P); Al(&n->msv, P); Al(&n->stats, 8);
    Al(&n->stats64, 4 + 2 * kA3cSumsqBlocks); Al(&n->kstep, E); Al(&n->ev_total, E); Al(&n->ev_len, E); Al(&n->ev_fin, E);
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

// The rollout of the nets whose temporal row is the whole processed observation (the Gaussian and the discrete agent; D = S0 =
// net->D, obs = the handle's processed observation): T steps of record, forward + action, env step, episode accounting and window
// rule; then V of the window after the last step, with always_bootstrap also V behind every finished episode (workgroups whose 64
// samples ended none leave at once), and the worker's GAE (worker.py:241-294).  The net brings what differs:
//   args(n, states, windows)   its forward's argument block (fields vals and gate are set here)
//   acting(a, o, t)            the heads' outputs and the action of step t into the rollout buffers at sample offset o = t * E
//   fwd(a)                     the forward launch
//   env_step(o)                the env's step on the actions recorded at o
// and the buffers ro_states .. ro_boot, boot_states, boot_win, term_obs by these names.
template <typename NET, typename ARGS, typename ACTING, typename FWD, typename STEP>
static int a3c_rollout_run(NET *net, int T, const float *obs, ARGS args, ACTING acting, FWD fwd, STEP env_step) {
    grl_handle *h = net->h;
    hipStream_t st = h->stream;
    const int E = h->E, R = net->cfg.rnn_length, D = net->D, eb = (E + 255) / 256, ab = net->cfg.always_bootstrap;
    const size_t TE = (size_t)T * E;
    int rc;
    if (ab) A3C_HIP(net, hipMemsetAsync(net->ro_term_val, 0, TE * 4, st));      // steps that end no episode read 0
    hipLaunchKernelGGL((a3c_sync_kernel<int, int, int>), dim3(eb), dim3(256), 0, st, h->elapsed, obs, net->win, net->kstep, E, R, D, D, 0, net->win_init ? 0 : 1);
    net->win_init = 1;
    for (int t = 0; t < T; ++t) {
        const size_t o = (size_t)t * E;
        hipLaunchKernelGGL((a3c_record_kernel<int, int>), dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, D, D, net->ro_states + o * D,
                           net->ro_win + o * R * D, net->ro_wt + o);
        auto a = args(E, net->ro_states + o * D, net->ro_win + o * R * D);
        a.vals = net->ro_val + o;
        acting(a, o, t);
        if ((rc = fwd(a))) return rc;
        if ((rc = env_step(o))) return a3c_fail(net, rc, h->err);
        if ((rc = episodes_launch_account(h))) return a3c_fail(net, rc, h->err);
        hipLaunchKernelGGL((a3c_post_kernel<int, int, int>), dim3(eb), dim3(256), 0, st, h->reward, h->done, obs, ab ? net->term_obs : (const float *)nullptr,
                           net->win, net->kstep, E, R, D, D, 0, net->ro_rew + o, net->ro_done + o, net->ro_mask + o,
                           ab ? net->ro_term_st + o * D : (float *)nullptr, ab ? net->ro_term_wn + o * R * D : (float *)nullptr);
    }
    if (!net->greedy) net->act_counter += (uint64_t)T;      // a greedy rollout draws nothing
    hipLaunchKernelGGL((a3c_record_kernel<int, int>), dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, D, D, net->boot_states, net->boot_win,
                       (float *)nullptr);
    auto b = args(E, net->boot_states, net->boot_win);
    b.vals = net->ro_boot;
    if ((rc = fwd(b))) return rc;
    if (ab) {
        auto c = args((int)TE, net->ro_term_st, net->ro_term_wn);
        c.gate = net->ro_done; c.vals = net->ro_term_val;
        if ((rc = fwd(c))) return rc;
    }
    hipLaunchKernelGGL(a3c_returns_kernel<float>, dim3(eb), dim3(256), 0, st, net->ro_rew, net->ro_val, net->ro_done, net->ro_term_val, net->ro_boot, T, E,
                       net->cfg.gamma, net->cfg.gae_lambda, net->cfg.scale, ab, net->ro_tgt, net->ro_adv);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// behind the evaluation kernel: the list and count of the handle's full reset, as grl_reset(h, NULL, 0) enqueues them; the caller
// then launches its env's reset on h->done_list / h->done_count
static int a3c_eval_finish(A3cNet *net, int trace_steps) {
    grl_handle *h = net->h;
    A3C_HIP(net, hipGetLastError());
    net->ev_trace = trace_steps;
    net->ev_played = -1;
    net->win_init = 0;      // the windows were the evaluation's: the next rollout starts every env's anew
    int rc = launch_iota(h, h->done_list, h->E);
    if (rc) return a3c_fail(net, rc, h->err);
    net->ev_reset_count = h->E;
    A3C_HIP(net, hipMemcpyAsync(h->done_count, &net->ev_reset_count, 4, hipMemcpyHostToDevice, h->stream));
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

// a device buffer by name; absent (null with a size): one the net's configuration does not keep
struct A3cBuf { const char *name; const void *p; size_t bytes; };

template <size_t N>
static int a3c_read(A3cNet *net, const char *fn, const A3cBuf (&tab)[N], const char *absent, const char *which, void *host, size_t bytes) {
    const A3cBuf *e = nullptr;
    for (const A3cBuf &b : tab)
        if (!strcmp(which, b.name)) e = &b;
    if (e && !e->p && e->bytes) return a3c_fail(net, GRL_E_STATE, std::string(fn) + ": " + which + absent);
    if (!e) return a3c_fail(net, GRL_E_INVALID, std::string(fn) + ": unknown buffer " + which);
    if (bytes != e->bytes) return a3c_fail(net, GRL_E_SIZE, std::string(fn) + ": wrong size for " + which);
    hipSetDevice(net->h->cfg.device_id);
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if (bytes) A3C_HIP(net, hipMemcpy(host, e->p, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // namespace grl
