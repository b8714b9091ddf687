// Evaluation of ConvSingleAgentPolicyNetwork on its Swarm handle, whole episodes without a host round trip (C ABI:
// include/goldsrl_neteval.h); included by net_conv.hip behind net_train.inc.  The forward pass is 6 MB of weights on MFMA GEMMs and
// cannot live inside one workgroup the way the field net's does (net_field_eval.inc), so an episode is not one kernel: it is the
// training rollout's pipeline (grl_net_rollout, net_train.inc) turned into an evaluation.  Per step and chunk of envs, on the
// chunk's lane: forward_chunk on the handle's observation -> eval_action_kernel -> swarm_launch_step_range (the step, the
// auto-reset, the next observation) -> eval_account_kernel; the lanes are forked once and joined once, and nothing is read back
// until grl_net_read_eval.  What a host loop pays per step -- a blocking predict, a draw, a transform, a step and four reads, 128
// times an episode -- is paid once.
//
// Nothing here restates the net or the env: the forward is forward_chunk, the step swarm_launch_step_range, and the action kernel's
// draw and clip are sample_actions_kernel's statements (net_conv.hip), so a drawn episode is the rollout's bit for bit up to the
// env's first done, and one with host normals the host loop's predict -> (mu + sigma z).astype(float32) -> transform_actions -> step.
//
// Left alone: parameters, optimizer state, the action counter, keep_version and the resident slots (every forward binds the chunk
// workspace, bind_activations(net, -1)), and every ro_* buffer -- the evaluation has its own env action rows.  The device's range
// flag as the call finds it (a rollout's verdict the gradient step has not read yet; nets on a device share the word) is put back
// by the first read.
#include <limits.h>

namespace grl {

struct EvalStep {
    const float *mu, *sigma, *vs;                 // the heads of the whole batch: (B,2) (B,2) (B)
    const double *normals;                        // (E,S,10,2) or null: the keyed draw
    const uint8_t *alive;                         // (E)
    float *envact, *actions;                      // (B,2); (E,S,10,2) or null
    float *tr_mu, *tr_sigma, *tr_raw, *tr_value;  // the traced env's rows
    int32_t *done_count;                          // the lane's counter: zeroed for the env step that follows on this stream
    uint64_t seed;
    uint32_t env_off, counter;                    // counter: the net's action counter + t
    int i0, n, S, t, greedy, trace_env;
};

// One lane per agent-sample of the chunk, samples [i0, i0 + n) of the batch.  The draw, the float32 rounding of the raw action and the
// norm clip are sample_actions_kernel's statements.  An env past its episode's end (alive == 0) is still given its action -- its
// auto-reset state goes on being stepped -- but nothing of it is kept.
__global__ void eval_action_kernel(EvalStep P) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *P.done_count = 0;
    if (i >= P.n) return;
    i += P.i0;
    const int env = i / 10, a = i - env * 10;
    const float2 m = reinterpret_cast<const float2 *>(P.mu)[i], s = reinterpret_cast<const float2 *>(P.sigma)[i];
    float2 r = m;
    if (!P.greedy) {
        double e0, e1;
        if (P.normals) {
            const double2 z = reinterpret_cast<const double2 *>(P.normals)[((size_t)env * P.S + P.t) * 10 + a];
            e0 = z.x; e1 = z.y;
        } else {
            normal_pair(rng_block(P.seed, (uint32_t)env + P.env_off, P.counter, RS_ACTION, a), e0, e1);
        }
        r = make_float2((float)((double)m.x + (double)s.x * e0), (float)((double)m.y + (double)s.y * e1));
    }
    const float2 raw = r;
    float d = sqrtf(r.x * r.x + r.y * r.y);
    if (d >= 1.0f) { r.x /= d; r.y /= d; }
    reinterpret_cast<float2 *>(P.envact)[i] = r;
    if (!P.alive[env]) return;
    if (P.actions) reinterpret_cast<float2 *>(P.actions)[((size_t)env * P.S + P.t) * 10 + a] = r;
    if (env == P.trace_env) {
        const size_t k = (size_t)P.t * 10 + a;
        reinterpret_cast<float2 *>(P.tr_mu)[k] = m;
        reinterpret_cast<float2 *>(P.tr_sigma)[k] = s;
        reinterpret_cast<float2 *>(P.tr_raw)[k] = raw;
        P.tr_value[k] = P.vs[i];
    }
}

// One lane per env of the chunk, behind its step: the float64 reward and the length while the episode runs; the step that reports
// done ends it.  (reward64 / done of an env are the step's, the auto-reset behind it leaves them: quirk Q6.)
__global__ void eval_account_kernel(const double *__restrict__ reward64, const uint8_t *__restrict__ done, int e0, int ne, int S, int t,
                                    double *__restrict__ rewards, int32_t *__restrict__ length, uint8_t *__restrict__ finished,
                                    uint8_t *__restrict__ alive) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const int env = e0 + i;
    if (!alive[env]) return;
    rewards[(size_t)env * S + t] = reward64[env];
    length[env] = t + 1;
    if (done[env]) { finished[env] = 1; alive[env] = 0; }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// grows one of the evaluation's buffers (the net's own: on its allocation list, freed with it); the old contents are dropped.
// The caller has drained the stream.
template <typename T>
static int eval_grow(grl_net *net, T **p, size_t count) {
    if (*p) {
        auto it = std::find(net->allocs.begin(), net->allocs.end(), (void *)*p);
        if (it != net->allocs.end()) net->allocs.erase(it);
        PAAC_HIP(net, hipFree(*p));
        *p = nullptr;
    }
    return paac_alloc(net, p, count);
}

static int eval_reserve(grl_net *net, size_t steps, size_t envs, size_t norm, size_t act, size_t trace) {
    NetEval &v = net->ev;
    int rc = GRL_OK;
    auto G = [&](auto **p, size_t cnt) { if (rc == GRL_OK) rc = eval_grow(net, p, cnt); };
    // a capacity reads 0 while its buffers are being replaced, and stays there when one of them fails
    if (steps > v.cap_steps) { v.cap_steps = 0; G(&v.rewards, steps); if (rc) return rc; v.cap_steps = steps; }
    if (envs > v.cap_envs) {
        v.cap_envs = 0; G(&v.length, envs); G(&v.finished, envs); G(&v.alive, envs); G(&v.envact, envs * 20);
        if (rc) return rc;
        v.cap_envs = envs;
    }
    if (norm > v.cap_norm) { v.cap_norm = 0; G(&v.normals, norm * 20); if (rc) return rc; v.cap_norm = norm; }
    if (act > v.cap_act) { v.cap_act = 0; G(&v.actions, act * 20); if (rc) return rc; v.cap_act = act; }
    if (trace > v.cap_trace) {
        v.cap_trace = 0; G(&v.tr_mu, trace * 20); G(&v.tr_sigma, trace * 20); G(&v.tr_raw, trace * 20); G(&v.tr_value, trace * 10);
        if (rc) return rc;
        v.cap_trace = trace;
    }
    return GRL_OK;
}

// the range flag the evaluation set aside goes back to the device (nothing to do when it was clear)
static int eval_restore_flag(grl_net *net) {
    NetEval &v = net->ev;
    if (v.flag_before) PAAC_HIP(net, hipMemcpy(range_flag_ptr(net), &v.flag_before, sizeof(int), hipMemcpyHostToDevice));
    v.flag_before = 0;
    return GRL_OK;
}

static int eval_enqueue(grl_net *net, int S, int greedy, bool drawn_host, bool keep, int trace_env) {
    grl_handle *h = net->h;
    NetEval &v = net->ev;
    const int E = h->E, ce = net->chunk / 10, nchunks = (E + ce - 1) / ce;
    const size_t steps = (size_t)E * S;
    PAAC_HIP(net, hipMemsetAsync(v.rewards, 0, steps * 8, h->stream));      // rows are written up to the env's length; the rest reads as zero
    PAAC_HIP(net, hipMemsetAsync(v.length, 0, (size_t)E * 4, h->stream));
    PAAC_HIP(net, hipMemsetAsync(v.finished, 0, (size_t)E, h->stream));
    PAAC_HIP(net, hipMemsetAsync(v.alive, 1, (size_t)E, h->stream));
    if (keep) PAAC_HIP(net, hipMemsetAsync(v.actions, 0, steps * 80, h->stream));
    if (trace_env >= 0) {
        float *rows[] = {v.tr_mu, v.tr_sigma, v.tr_raw};
        for (float *p : rows) PAAC_HIP(net, hipMemsetAsync(p, 0, (size_t)S * 80, h->stream));
        PAAC_HIP(net, hipMemsetAsync(v.tr_value, 0, (size_t)S * 40, h->stream));
    }
    // the lanes, as grl_net_rollout deals them: chunk c always runs on lane c % nl, one fork (behind the fills above), one join
    LanePass pass(net);
    int rc = pass.begin();
    if (rc) return rc;
    const int nl = lanes_active(net);
    net->side_now = nchunks == 1;      // one chunk per step: lane 0's side stream takes the forward's index kernels
    SideOff side_off{net};
    EvalStep P{};
    P.mu = net->mu; P.sigma = net->sigma; P.vs = net->vs;
    P.normals = drawn_host ? v.normals : nullptr;
    P.alive = v.alive; P.envact = v.envact; P.actions = keep ? v.actions : nullptr;
    P.tr_mu = v.tr_mu; P.tr_sigma = v.tr_sigma; P.tr_raw = v.tr_raw; P.tr_value = v.tr_value;
    P.seed = h->cfg.seed; P.env_off = (uint32_t)h->cfg.env_id_offset;
    P.S = S; P.greedy = greedy; P.trace_env = trace_env;
    for (int t = 0; t < S; ++t)
        for (int c = 0; c < nchunks; ++c) {
            const int e0 = c * ce, ne = E - e0 < ce ? E - e0 : ce;
            use_lane(net, c % nl);
            net->last_lane = net->cur_lane;
            hipStream_t st = h->stream;      // the lane's stream
            bind_activations(net, -1);
            rc = forward_chunk(net, h->sw.lbins + (size_t)e0 * 160, h->sw.abins + (size_t)e0 * 20, h->sw.pos + (size_t)e0 * 20, ne,
                               net->mu + (size_t)e0 * 20, net->sigma + (size_t)e0 * 20, net->vs + (size_t)e0 * 10);
            if (rc) return rc;
            P.i0 = e0 * 10; P.n = ne * 10; P.t = t;
            P.counter = (uint32_t)(net->act_counter + (unsigned long)t);      // the rollout's key; the counter itself stays
            P.done_count = h->done_count + net->cur_lane;
            hipLaunchKernelGGL(eval_action_kernel, dim3((ne * 10 + 255) / 256), dim3(256), 0, st, P);
            if ((rc = swarm_launch_step_range(h, v.envact, e0, ne, net->cur_lane, true))) return paac_fail(net, rc, h->err);
            hipLaunchKernelGGL(eval_account_kernel, dim3((ne + 255) / 256), dim3(256), 0, st, (const double *)h->sw.reward64, (const uint8_t *)h->done, e0,
                               ne, S, t, v.rewards, v.length, v.finished, v.alive);
        }
    if ((rc = pass.finish())) return rc;
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_net_eval(grl_net *net, int32_t max_steps, int32_t greedy, const double *normals_host, int32_t keep_actions, int32_t trace_env) {
    const std::string fn = "grl_net_eval";
    if (!net) return GRL_E_INVALID;
    grl_handle *h = net->h;
    if (max_steps < 1 || max_steps > 1024) return paac_fail(net, GRL_E_INVALID, fn + ": max_steps must be in 1..1024");
    if (net->ho.A != 2) return paac_fail(net, GRL_E_INVALID, fn + ": SwarmEnv.step takes (10, 2) actions; this net was built with num_actions != 2");
    if (trace_env < -1 || trace_env >= h->E) return paac_fail(net, GRL_E_INVALID, fn + ": trace_env must be -1 or an env index");
    if (normals_host && greedy) return paac_fail(net, GRL_E_INVALID, fn + ": a greedy evaluation draws nothing (normals_host with greedy)");
    if (h->step_in_flight) return paac_fail(net, GRL_E_INVALID, fn + ": a step is in flight (grl_wait first)");
    const size_t E = (size_t)h->E, steps = E * max_steps, largest = (keep_actions || normals_host) ? steps * 20 : steps;
    if (largest > (size_t)INT32_MAX)
        return paac_fail(net, GRL_E_INVALID, fn + ": an output of " + std::to_string(largest) + " elements does not fit in int32 (fewer envs or steps per call)");
    hipSetDevice(h->cfg.device_id);
    NetEval &v = net->ev;
    v.max_steps = 0;
    PAAC_HIP(net, hipStreamSynchronize(h->stream));      // idle already (no step in flight); what follows frees, copies and reads
    if (v.unchecked) {      // an evaluation nobody read: its flag is nobody's verdict
        PAAC_HIP(net, hipMemset(range_flag_ptr(net), 0, sizeof(int)));
        v.unchecked = false;
        if (int rc = eval_restore_flag(net)) return rc;
    }
    int rc = eval_reserve(net, steps, E, normals_host ? steps : 0, keep_actions ? steps : 0, trace_env >= 0 ? (size_t)max_steps : 0);
    if (rc) return rc;
    if (normals_host) PAAC_HIP(net, hipMemcpy(v.normals, normals_host, steps * 160, hipMemcpyHostToDevice));
    // A rollout's verdict on itself (bit 2, rollout_range_mark_kernel) waits for the gradient step: set aside, so that the first read
    // sees this evaluation's forward passes, and put back behind it.  A flag nobody marked (1: a background pass of the parameters
    // just uploaded) stays and is this evaluation's to report, as it would be the next predict's.
    PAAC_HIP(net, hipMemcpy(&v.flag_before, range_flag_ptr(net), sizeof(int), hipMemcpyDeviceToHost));
    if (v.flag_before & 2) PAAC_HIP(net, hipMemset(range_flag_ptr(net), 0, sizeof(int)));
    else v.flag_before = 0;
    rc = eval_enqueue(net, max_steps, greedy ? 1 : 0, normals_host != nullptr, keep_actions != 0, trace_env);
    if (rc) {      // part of it may be on the streams (joined into the handle's): drained before the flag word is touched
        (void)hipStreamSynchronize(h->stream);
        (void)hipMemset(range_flag_ptr(net), 0, sizeof(int));
        (void)eval_restore_flag(net);
        return rc;
    }
    v.max_steps = max_steps; v.trace_env = trace_env; v.keep_actions = keep_actions ? 1 : 0;
    v.unchecked = true;
    h->step_in_flight = true;
    return GRL_OK;
}

int grl_net_read_eval(grl_net *net, const char *which, void *host, size_t bytes) {
    const std::string fn = "grl_net_read_eval";
    if (!net) return GRL_E_INVALID;
    if (!which || !host) return paac_fail(net, GRL_E_INVALID, fn + ": null argument");
    grl_handle *h = net->h;
    NetEval &v = net->ev;
    if (!v.max_steps) return paac_fail(net, GRL_E_STATE, fn + ": no evaluation to read (grl_net_eval first; one that left the fp16 range is run again)");
    const size_t E = (size_t)h->E, S = (size_t)v.max_steps;
    const char *untraced = v.trace_env < 0 ? "the last evaluation traced no env (trace_env was -1)" : nullptr;
    const struct { const char *name; const void *src; size_t bytes; const char *absent; } outs[] = {
        {"rewards", v.rewards, E * S * 8, nullptr}, {"length", v.length, E * 4, nullptr}, {"finished", v.finished, E, nullptr},
        {"actions", v.actions, E * S * 80, v.keep_actions ? nullptr : "the last evaluation kept no actions (keep_actions was 0)"},
        {"trace_mu", v.tr_mu, S * 80, untraced}, {"trace_sigma", v.tr_sigma, S * 80, untraced}, {"trace_raw", v.tr_raw, S * 80, untraced},
        {"trace_value", v.tr_value, S * 40, untraced}};
    const std::string s(which);
    const auto *o = &outs[0];
    bool found = false;
    for (const auto &e : outs)
        if (s == e.name) { o = &e; found = true; }
    if (!found) return paac_fail(net, GRL_E_INVALID, fn + ": unknown output '" + s + "'");
    if (o->absent) return paac_fail(net, GRL_E_STATE, fn + ": " + o->absent);
    if (o->bytes != bytes) return paac_fail(net, GRL_E_SIZE, fn + ": '" + s + "' needs " + std::to_string(o->bytes) + " bytes, got " + std::to_string(bytes));
    hipSetDevice(h->cfg.device_id);
    PAAC_HIP(net, hipStreamSynchronize(h->stream));      // the lanes were joined into it
    if (v.unchecked) {      // the first read behind the evaluation (the handle's in-flight mark stays grl_wait's, as behind a rollout)
        v.unchecked = false;
        int rc = range_check(net, "grl_net_eval");      // reads the word, and clears it when it is set
        const int rrc = eval_restore_flag(net);
        if (rc == GRL_E_RANGE) {
            v.max_steps = 0;      // actions from invalid heads: nothing of this evaluation is handed out
            const std::string msg = net->err;
            (void)range_fall_back(net);      // GRL_NET_RANGE_FALLBACK=off: the net stays where it is
            PAAC_HIP(net, hipStreamSynchronize(h->stream));
            return paac_fail(net, GRL_E_RANGE, msg + (net->gemm_f32 ? "; the net is on the fp32 form now: reset the env and evaluate again" : ""));
        }
        if (rc) return rc;
        if (rrc) return rrc;
    }
    PAAC_HIP(net, hipMemcpy(host, o->src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // extern "C"
