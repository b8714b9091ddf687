// The host scaffold the three PAAC nets share (grl_net: net_conv.hip + net_train.inc, grl_fnet: net_flat.hip, grl_fieldnet:
// net_field.hip): the state their handles derive from and one copy of what they do alike -- the error slot, the allocation list,
// the flat copies with their size check, optimizer state and action counter, the RCCL communicator with the gradient all-reduce
// and its timing, Adam's step size, the stats read-back, teardown -- plus the two update kernels that were the same text.
// Included behind common.h; static: every including translation unit has its own copy.  Functions take the C
// function's name where their message carries it (nullptr: the bare message).
#pragma once

#include <rccl/rccl.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

namespace grl {

struct PaacNet {
    grl_handle *h = nullptr;
    std::string err;
    int64_t num_params = 0;
    float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    float *stats = nullptr;        // device: [0..1] loss parts (mean), [2] loss, [3] global norm, [4] clip factor; behind them the net's own
    long adam_t = 0;
    unsigned long act_counter = 0;
    bool alloc_waits = false;      // paac_alloc finishes its fill before it returns (the conv net's lanes)
    std::vector<void *> allocs;
};

// the two nets that train over ranks: one all-reduce of the flat gradient per rollout
struct PaacCommNet : PaacNet {
    void *comm = nullptr;          // ncclComm_t (RCCL), or nullptr
    int comm_world = 1, comm_rank = 0;
    hipEvent_t ar_ev0 = nullptr, ar_ev1 = nullptr;      // bracket the all-reduce on the handle's stream (grl_*_comm_info)
    int ar_pending = 0;
    long ar_calls = 0;
    double ar_ms_total = 0.0;
    float ar_ms_last = 0.f;
};

static int paac_fail(PaacNet *n, int code, const std::string &msg) {
    if (n) n->err = msg;
    return code;
}
#define PAAC_HIP(n, call)                                                                                      \
    do {                                                                                                       \
        hipError_t _e = (call);                                                                                \
        if (_e != hipSuccess) return paac_fail(n, GRL_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
static int paac_alloc(PaacNet *n, T **p, size_t count) {
    PAAC_HIP(n, hipMalloc((void **)p, count * sizeof(T)));
    n->allocs.push_back(*p);
    PAAC_HIP(n, hipMemsetAsync(*p, 0, count * sizeof(T), n->h->stream));
    // the conv net allocates on whichever lane is current (a non-blocking stream) while other streams may be the first to touch the
    // buffer (w2t / w3t are written on the main stream): finish the fill before anyone can see the pointer
    if (n->alloc_waits) PAAC_HIP(n, hipStreamSynchronize(n->h->stream));
    return GRL_OK;
}

static const char *paac_last_error(const PaacNet *n) { return n ? n->err.c_str() : ""; }
static int64_t paac_num_params(const PaacNet *n) { return n ? n->num_params : 0; }

// a flat vector of num_params floats (parameters, gradient, Adam moment) to or from the host
static int paac_copy_flat(PaacNet *n, const char *fn, float *dev, float *host, int64_t cnt, bool to_dev) {
    if (!n || !host) return GRL_E_INVALID;
    if (cnt != n->num_params)
        return paac_fail(n, GRL_E_SIZE, (fn ? std::string(fn) + ": " : std::string()) + "expected " + std::to_string((long)n->num_params) + " floats");
    hipSetDevice(n->h->cfg.device_id);
    PAAC_HIP(n, hipStreamSynchronize(n->h->stream));
    if (to_dev) PAAC_HIP(n, hipMemcpy(dev, host, cnt * 4, hipMemcpyHostToDevice));
    else PAAC_HIP(n, hipMemcpy(host, dev, cnt * 4, hipMemcpyDeviceToHost));
    return GRL_OK;
}

static int paac_get_optimizer_state(PaacNet *n, float *m_host, float *v_host, int64_t cnt, int64_t *step_out) {
    if (!n || !m_host || !v_host || !step_out) return GRL_E_INVALID;
    int rc = paac_copy_flat(n, nullptr, n->adam_m, m_host, cnt, false);
    if (rc == GRL_OK) rc = paac_copy_flat(n, nullptr, n->adam_v, v_host, cnt, false);
    *step_out = n->adam_t;
    return rc;
}

static int paac_set_optimizer_state(PaacNet *n, const char *fn, const float *m_host, const float *v_host, int64_t cnt, int64_t step) {
    if (!n || !m_host || !v_host || step < 0) return GRL_E_INVALID;
    int rc = paac_copy_flat(n, fn, n->adam_m, (float *)m_host, cnt, true);
    if (rc == GRL_OK) rc = paac_copy_flat(n, fn, n->adam_v, (float *)v_host, cnt, true);
    if (rc == GRL_OK) n->adam_t = (long)step;
    return rc;
}

static int paac_get_action_counter(PaacNet *n, uint64_t *out) {
    if (!n || !out) return GRL_E_INVALID;
    *out = (uint64_t)n->act_counter;
    return GRL_OK;
}

static int paac_set_action_counter(PaacNet *n, uint64_t value) {
    if (!n) return GRL_E_INVALID;
    n->act_counter = (unsigned long)value;
    return GRL_OK;
}

// ---- the communicator
static int paac_comm_init(PaacCommNet *net, const char *fn, const void *unique_id, size_t bytes, int32_t rank, int32_t world_size) {
    if (!net || !unique_id || bytes != sizeof(ncclUniqueId) || world_size < 1 || rank < 0 || rank >= world_size)
        return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": bad argument");
    if (net->comm) return paac_fail(net, GRL_E_STATE, std::string(fn) + ": communicator already attached");
    hipSetDevice(net->h->cfg.device_id);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm;
    ncclResult_t r = ncclCommInitRank(&comm, world_size, id, rank);
    (void)hipGetLastError();
    if (r != ncclSuccess) return paac_fail(net, GRL_E_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    net->comm = (void *)comm; net->comm_world = world_size; net->comm_rank = rank;
    return GRL_OK;
}

static int paac_comm_info(PaacCommNet *net, int32_t *count_out, int32_t *user_rank_out, int64_t *allreduce_calls_out,
                          double *allreduce_ms_total_out, float *allreduce_ms_last_out) {
    if (!net) return GRL_E_INVALID;
    int count = 0, urank = -1;
    if (net->comm) {
        ncclResult_t r = ncclCommCount((ncclComm_t)net->comm, &count);
        if (r == ncclSuccess) r = ncclCommUserRank((ncclComm_t)net->comm, &urank);
        (void)hipGetLastError();
        if (r != ncclSuccess) return paac_fail(net, GRL_E_COMM, std::string("ncclCommCount: ") + ncclGetErrorString(r));
    }
    if (count_out) *count_out = count;
    if (user_rank_out) *user_rank_out = urank;
    if (allreduce_calls_out) *allreduce_calls_out = net->ar_calls;
    if (allreduce_ms_total_out) *allreduce_ms_total_out = net->ar_ms_total;
    if (allreduce_ms_last_out) *allreduce_ms_last_out = net->ar_ms_last;
    return GRL_OK;
}

// root's parameters to every rank, waited for; what follows a move of the parameters is the caller's
static int paac_comm_broadcast_params(PaacCommNet *net, const char *fn, int32_t root) {
    if (!net || !net->comm) return paac_fail(net, GRL_E_STATE, std::string(fn) + ": no communicator");
    hipSetDevice(net->h->cfg.device_id);
    ncclResult_t r = ncclBroadcast(net->params, net->params, (size_t)net->num_params, ncclFloat, root, (ncclComm_t)net->comm, net->h->stream);
    (void)hipGetLastError();
    if (r != ncclSuccess) return paac_fail(net, GRL_E_COMM, std::string("ncclBroadcast: ") + ncclGetErrorString(r));
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    return GRL_OK;
}

static int paac_comm_destroy(PaacCommNet *net) {
    if (!net) return GRL_E_INVALID;
    if (net->comm) {
        hipSetDevice(net->h->cfg.device_id);
        hipStreamSynchronize(net->h->stream);
        ncclCommDestroy((ncclComm_t)net->comm);
        (void)hipGetLastError();
        net->comm = nullptr; net->comm_world = 1; net->comm_rank = 0;
    }
    return GRL_OK;
}

// One all-reduce (sum, fp32) of the flat gradient per rollout over RCCL/xGMI.  Every rank's gradient is the mean over
// ITS samples; the reference's loss is a mean over the whole batch (policy_v_network.py:54,62 / 246-251), so the summed gradient is
// scaled by 1/world afterwards (grad_scale, folded into the clip factor); clip-by-global-norm is applied after the reduction, Adam
// runs replicated.  max_words: two uint32 words that travel with the gradient by max, grouped with it (the conv net's range
// words), or nullptr.  Bracketed by HIP events on the handle's stream; paac_allreduce_account reads them once the stream is idle.
static int paac_allreduce_grads(PaacCommNet *net, float *grads, void *max_words, float *grad_scale_out) {
    *grad_scale_out = 1.0f;
    if (!net->comm) return GRL_OK;
    hipStream_t st = net->h->stream;
    ncclComm_t comm = (ncclComm_t)net->comm;
    if (!net->ar_ev0) { PAAC_HIP(net, hipEventCreate(&net->ar_ev0)); PAAC_HIP(net, hipEventCreate(&net->ar_ev1)); }
    PAAC_HIP(net, hipEventRecord(net->ar_ev0, st));
    ncclResult_t r = max_words ? ncclGroupStart() : ncclSuccess;
    if (max_words && r == ncclSuccess) r = ncclAllReduce(max_words, max_words, 2, ncclUint32, ncclMax, comm, st);
    if (r == ncclSuccess) r = ncclAllReduce(grads, grads, (size_t)net->num_params, ncclFloat, ncclSum, comm, st);
    if (max_words) {
        ncclResult_t r2 = ncclGroupEnd();
        if (r == ncclSuccess) r = r2;
    }
    (void)hipGetLastError();   // RCCL probes (peer access, other ordinals) may leave a stale HIP error on this thread
    if (r != ncclSuccess) return paac_fail(net, GRL_E_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    PAAC_HIP(net, hipEventRecord(net->ar_ev1, st));
    net->ar_pending = 1;
    *grad_scale_out = 1.0f / (float)net->comm_world;
    return GRL_OK;
}

static void paac_allreduce_account(PaacCommNet *net) {
    if (!net->ar_pending) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, net->ar_ev0, net->ar_ev1) == hipSuccess) { net->ar_ms_last = ms; net->ar_ms_total += ms; net->ar_calls += 1; }
    net->ar_pending = 0;
}

// ---- the update.  The two kernels are templates so that a translation unit holds only the one it launches.
// sum of squares in float64 in a fixed order: gridDim.x strided partial sums (tree inside the block), added up in order by the
// net's finalize kernel
template <int BLOCK = 256>
__global__ __launch_bounds__(BLOCK) void paac_sumsq_kernel(const float *__restrict__ g, long n, double *__restrict__ partial) {
    __shared__ double red[BLOCK];
    double s = 0.0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) s += (double)g[i] * (double)g[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// tf.train.AdamOptimizer (TF 1.4): m, v update, p -= lr_t * m / (sqrt(v) + eps), lr_t folded on the host; stats[4] = the clip factor.
// The one Adam arithmetic of the tree: beta1, 1 - beta1, beta2, 1 - beta2 and eps are the float32 literals below (1.0f - 0.999f
// computed in float32 is 1.3e-5 low, relative: 216 roundings of v).
// range_flag (nullptr: no check): the sticky fp16-range flag of the conv net's GEMMs (net_gemm.h).  When it is set the gradient of
// this pass was computed from inf / NaN operands: the update is skipped ON THE DEVICE, so the call that then fails with
// GRL_E_RANGE leaves the parameters and the Adam moments exactly as they were (with ranks the flag is max-reduced next to the
// gradient: every replica skips together).
template <typename F = float>
__global__ void paac_adam_kernel(F *__restrict__ p, const F *__restrict__ g, F *__restrict__ m, F *__restrict__ v, long n,
                                 const float *__restrict__ stats, float lr_t, const int *__restrict__ range_flag = nullptr) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (range_flag && *range_flag)) return;
    float gi = g[i] * stats[4];
    float mi = 0.9f * m[i] + 0.1f * gi;
    float vi = 0.999f * v[i] + 0.001f * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + 1e-8f);
}

// Adam's step size at update t (t >= 1): lr * sqrt(1 - b2^t) / (1 - b1^t)
static float adam_lr_t(float lr, long t) { return (float)((double)lr * sqrt(1.0 - pow(0.999, (double)t)) / (1.0 - pow(0.9, (double)t))); }

// [loss, policy loss, critic loss, global norm] of the update just waited for
static int paac_read_stats(PaacNet *n, float *stats_host) {
    if (!stats_host) return GRL_OK;
    float s[5];
    PAAC_HIP(n, hipMemcpy(s, n->stats, sizeof(s), hipMemcpyDeviceToHost));
    stats_host[0] = s[2]; stats_host[1] = s[0]; stats_host[2] = s[1]; stats_host[3] = s[3];
    return GRL_OK;
}

// ---- destroy: the communicator with its events, then (after whatever else the net owns) the allocation list
static void paac_comm_release(PaacCommNet *n) {
    if (n->comm) {
        ncclCommDestroy((ncclComm_t)n->comm);
        (void)hipGetLastError();   // RCCL teardown may leave a stale HIP error on this thread
    }
    if (n->ar_ev0) { hipEventDestroy(n->ar_ev0); hipEventDestroy(n->ar_ev1); }
}

static void paac_free(PaacNet *n) {
    for (void *p : n->allocs) hipFree(p);
}

}  // namespace grl
