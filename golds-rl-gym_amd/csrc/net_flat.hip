// FlatPolicyVNetwork on gfx950 (reference fed_gym/agents/paac/policy_v_network.py:194-264 with the GRU
// trunk of fed_gym/agents/a3c/estimators.py:5-28), its loss/backward/optimiser and the flat PAAC rollout
// (fed_gym/agents/paac/paac.py:119-187) for Solow handles and, PAAC-style, TradeAR1 handles (BASELINE config 5:
// obs transform of a3c/worker.py:420-431, tanh actions :440-442, hyper-parameters of scripts/train_trade.py:38-40,119).
//
// The net has ~31k parameters and a few tens of kMAC per sample; BASELINE config 2 (4 096 envs) is
// launch/latency bound, so the whole forward (5 GRU steps + 13 dense layers) is ONE launch and the
// whole backward one more.  A workgroup of 4 waves owns 64 samples; activations are staged in LDS as
// [feature][sample] (row stride 65) and every dense layer and every gradient is a small fp32 MFMA GEMM against
// those rows (net_flat_mfma.inc).  Weight gradients are summed per workgroup into private slabs and reduced in
// a fixed order (bitwise reproducible).
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/goldsrl_flatnet.h"      // brings goldsrl_flateval.h and goldsrl_flatwindow.h
#include "common.h"
#include "net_paac_host.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "rollout_dev.h"

namespace grl {

constexpr int FH = 32;       // rnn hidden (and static hidden)
constexpr int LS = 65;       // LDS row stride
constexpr int MAXD = 33;     // temporal_size <= 33 (TradeAR1-16: 1+2n)
constexpr int MAXS0 = 64;
constexpr int MAXA = 16;
enum : uint32_t { RS_FLAT_ACTION = 17 };

struct FOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, m1w, m1b, m2w, m2b, m3w, m3b, g1w, g1b, g2w, g2b, g3w, g3b, v1w, v1b, v2w, v2b, total;
};

static FOff make_offsets(int D, int S0, int A) {
    FOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((long)(D + FH) * 2 * FH); o.gb = take(2 * FH);
    o.cw = take((long)(D + FH) * FH); o.cb = take(FH);
    o.tw = take(FH * 2 * FH); o.tb = take(2 * FH);
    o.s1w = take((long)S0 * 2 * FH); o.s1b = take(2 * FH);
    o.s2w = take(2 * FH * FH); o.s2b = take(FH);
    o.m1w = take(3 * FH * 2 * FH); o.m1b = take(2 * FH); o.m2w = take(2 * FH * FH); o.m2b = take(FH); o.m3w = take((long)FH * A); o.m3b = take(A);
    o.g1w = take(3 * FH * 2 * FH); o.g1b = take(2 * FH); o.g2w = take(2 * FH * FH); o.g2b = take(FH); o.g3w = take((long)FH * A); o.g3b = take(A);
    o.v1w = take(3 * FH * 2 * FH); o.v1b = take(2 * FH); o.v2w = take(2 * FH); o.v2b = take(1);
    o.total = p;
    return o;
}

// workspace features per sample: per GRU step {h_prev, r, u, c} then the dense activations.
// Layout [group of 64 samples][feature][64] (ws_row): the ~3 000 rows a group's backward reads are one contiguous block of 0.8 MB.
// As [feature][n] they lay n * 4 bytes apart -- 655 KB at 8 192 envs x 20 steps, every row of a tile on another page.
__host__ __device__ inline int ws_step(int t) { return t * 4 * FH; }
struct WsOff { int dt, s1, s2, m1, m2, tm, g1, g2, sg, v1, hl, vs, total; };
__host__ __device__ inline WsOff ws_offsets(int T, int A) {
    WsOff w;
    int p = T * 4 * FH;
    w.dt = p; p += 64; w.s1 = p; p += 64; w.s2 = p; p += 32; w.m1 = p; p += 64; w.m2 = p; p += 32; w.tm = p; p += A;
    w.g1 = p; p += 64; w.g2 = p; p += 32; w.sg = p; p += A; w.v1 = p; p += 64; w.hl = p; p += 32; w.vs = p; p += 1;
    w.total = p;
    return w;
}
// row `f` of the group that starts at sample sbase (a multiple of 64): 64 floats
__host__ __device__ inline float *ws_row(float *ws, int f, int sbase, int F) { return ws + ((size_t)(sbase >> 6) * F + f) * 64; }
__host__ __device__ inline const float *ws_row(const float *ws, int f, int sbase, int F) { return ws + ((size_t)(sbase >> 6) * F + f) * 64; }

struct FlatArgs {
    const float *P;
    const float *PT;                // backward only: every [K][N] weight matrix as [N][K] at the same offset (flat_transpose_kernel)
    FOff o;
    int n, S0, D, T, A;
    float scale, bound;
    const float *states, *hist;     // (n,S0) (n,T,D) row-major
    const int32_t *nhist;           // if set: hist is NOT read; row t of sample s is states[s] for t < min(nhist[s],T), else 0
                                    // (the PAAC worker's window, quirk Q11; needs D == S0)
    float *mu, *sigma, *vs;         // (n,A) (n,A) (n)
    float *ws;                      // [feature][n] or nullptr (inference)
    // backward only
    const float *actions, *adv, *y;
    float inv_n;
    float *slab;                    // [blocks][o.total]
    double *stats64;
    long long *ts;                  // stage clock of workgroup 0 (debug, grl_fnet_rollout_stage_times) or nullptr
    int *ts_n;
    int wstride, wring;             // wstride > 0: the TRUE window (net_flat_window.inc) -- nhist[s] rows wstride * S0 floats apart that end at
                                    // states[s]; wring > 0 (evaluation): the time slices form a ring of wring
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

#include "net_flat_mfma.inc"
#include "net_flat_fast.inc"
#include "net_flat_bwd_fast.inc"
#include "net_flat_rollout.inc"
#include "net_flat_eval.inc"
#include "net_flat_window.inc"

// PT: the weight matrices the data gradients multiply with, transposed (block b = matrix b; the GRU kernels: their recurrent rows)
__global__ void flat_transpose_kernel(const float *__restrict__ P, float *__restrict__ PT, FOff o, int D, int A) {
    long off;
    int K, N;
    switch (blockIdx.x) {
        case 0: off = o.m1w; K = 3 * FH; N = 2 * FH; break;
        case 1: off = o.g1w; K = 3 * FH; N = 2 * FH; break;
        case 2: off = o.v1w; K = 3 * FH; N = 2 * FH; break;
        case 3: off = o.m2w; K = 2 * FH; N = FH; break;
        case 4: off = o.g2w; K = 2 * FH; N = FH; break;
        case 5: off = o.m3w; K = FH; N = A; break;
        case 6: off = o.g3w; K = FH; N = A; break;
        case 7: off = o.tw; K = FH; N = 2 * FH; break;
        case 8: off = o.s2w; K = 2 * FH; N = FH; break;
        case 9: off = o.cw + (long)D * FH; K = FH; N = FH; break;
        default: off = o.gw + (long)D * 2 * FH; K = FH; N = 2 * FH; break;
    }
    for (int e = threadIdx.x; e < K * N; e += blockDim.x) {
        const int i = e / N, c = e - i * N;
        PT[off + (long)c * K + i] = P[off + e];
    }
}
constexpr int kFlatTransposed = 11;

// sum of squares in float64: kSumsqBlocks partial sums (a contiguous slice each, tree inside the block), added up in order by
// flat_finalize_kernel
constexpr int kSumsqBlocks = 32;
__global__ __launch_bounds__(256) void flat_sumsq_kernel(const float *__restrict__ g, long n, double *__restrict__ out) {
    __shared__ double red[256];
    const long per = (n + kSumsqBlocks - 1) / kSumsqBlocks, lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += (double)g[i] * (double)g[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// grad_scale: 1/world after a sum over ranks (the loss is a mean over the WHOLE batch, policy_v_network.py:246-251); the norm and
// the clip are those of grad_scale * grads, and the factor is folded into what Adam multiplies the stored gradient by
__global__ void flat_finalize_kernel(const double *__restrict__ sumsq, const double *__restrict__ stats64, float inv_n, float inv_na,
                                     float clip_norm, float grad_scale, float *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double ss = 0.0;
    for (int b = 0; b < kSumsqBlocks; ++b) ss += sumsq[b];
    float norm = (float)(sqrt(ss) * (double)grad_scale);
    float pl = (float)(stats64[0] * (double)inv_na), cl = (float)(stats64[1] * (double)inv_n);
    stats[0] = pl; stats[1] = cl; stats[2] = pl + cl; stats[3] = norm;
    stats[4] = grad_scale * (clip_norm > 0.f ? clip_norm / fmaxf(norm, clip_norm) : 1.0f);      // tf.clip_by_global_norm
}

// a = mu + sigma*N(0,1) (paac.py:36), SolowRunner.transform_actions_for_env = sigmoid (emulator_runner.py:77-79)
__global__ void flat_sample_kernel(const float *__restrict__ mu, const float *__restrict__ sigma, int n, int A, uint64_t seed,
                                   uint32_t env_off, const uint32_t *__restrict__ counter_base, uint32_t step, int env_kind, int greedy,
                                   float *__restrict__ raw, float *__restrict__ envact) {
    // the draw counter is read from device memory so that a captured rollout graph can be replayed (base is set per rollout)
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * A) return;
    const uint32_t counter = *counter_base + step;
    int e = i / A, k = i - e * A;
    const float r = flat_raw_action(greedy, mu[i], sigma[i], seed, (uint32_t)e + env_off, counter, k);
    raw[i] = r;
    envact[i] = flat_env_action(env_kind, r);
}

__global__ void flat_mask_kernel(const uint8_t *__restrict__ done, int n, float *__restrict__ mask) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mask[i] = 1.0f - (float)done[i];      // episodes_over_masks (paac.py:140)
}

}  // namespace grl

struct grl_fnet : grl::PaacCommNet {
    grl_fnet_config cfg;
    grl::FOff off;
    grl::WsOff wso;
    float *paramsT, *grads;      // paramsT: net_flat_bwd_fast.inc (fb_dx)
    float *ws, *slab;
    double *stats64;
    float *d_states, *d_hist, *d_act, *d_adv, *d_y, *mu, *sigma, *vs;
    int slab_blocks;
    // rollout
    int T;
    float *ro_states, *ro_hist, *ro_act, *ro_envact, *ro_val, *ro_rew, *ro_mask, *ro_y, *ro_adv, *ro_boot;
    int32_t *ro_nhist;
    uint32_t *d_counter;           // act_counter at the start of the rollout in flight
    hipGraphExec_t ro_graph;       // the T-step rollout captured once and replayed (launch-bound at 4 096 envs)
    int ro_graph_T;
    bool ro_graph_ep;              // the captured rollout contains the R6 accounting launches
    int ro_graph_greedy;           // the greedy flag the captured sample launches carry
    int greedy;                    // grl_fnet_set_greedy: the rollout acts with raw = mu, draws nothing, the action counter stands still
    // grl_fnet_eval: per-env results and the trace of the first ev_trace steps (buffers for ev_trace_cap steps; they only grow)
    double *ev_total;
    int32_t *ev_len, *ev_nhist;
    uint8_t *ev_fin;
    float *ev_states, *ev_mu, *ev_sigma, *ev_raw, *ev_act, *ev_val, *ev_rew, *ev_done;
    int ev_trace, ev_trace_cap, ev_played;      // ev_played: -1 until grl_fnet_read_eval has looked, -2 before any evaluation
    int32_t ev_reset_count;
    char ev_attr_set[3];           // flat_eval_kernel<16 / 32 / 64> has its dynamic-LDS limit raised on this net's device
    std::vector<void *> ev_allocs;
    int fast_forward;              // 1: synthesized-window forwards use net_flat_fast.inc (GRL_FLAT_FORWARD=layers: the layer-by-layer form)
    int ro_persistent;             // 1: the T-step actor loop is ONE persistent kernel (net_flat_rollout.inc); 0: the hipGraph of launches
    char ro_attr_set[2][3];        // the rollout kernel instance (KEEP x G = 16, 32, 64) has its dynamic-LDS limit raised on this net's device
    int ro_group;                  // envs per workgroup of the persistent rollout; 0: by the env count (GRL_FLAT_GROUP)
    int keep_activations;          // grl_fnet_set_keep_activations: the persistent rollout fills the training workspace
    int ws_resident;               // the workspace holds the forward of the last rollout's T x E samples under the CURRENT parameters
    int arg_slot;                  // this net's slot of g_flat_args (net_flat_fast.inc), -1: none free (graph path)
    long long *d_ts;               // stage timestamps of workgroup 0 of the persistent rollout (debug: grl_fnet_rollout_stage_times)
    int *d_ts_n;
    // grl_fnet_set_true_window (net_flat_window.inc): the rollout's states live in a slab with rnn - 1 leading time slices (and one
    // behind, the bootstrap observation), ro_states = ro_slab + (rnn - 1) * E * S0, and the windows are strided views of it
    int true_window;
    float *ro_slab;
    int slab_T;                    // rollout steps the slab has room for
    int32_t *w_len, *w_elapsed, *w_episode;      // (E): the rows the next forward sees; TimeLimit counter / episode the net saw last
    const float *w_src;            // where the rnn - 1 slices behind the next rollout's first step lie (ro_slab itself once carried)
    int w_restart_all, w_have;     // every window restarts at the next call; w_len / w_elapsed / w_episode describe a finished rollout
    int w_valid;                   // the slab still holds the last rollout (nothing was carried forward since)
    float *ev_ring;                // evaluation: (rnn, E, S0) ring of the last states
    char ro_win_attr_set[3], ev_win_attr_set[3];
    int ro_graph_tw;               // the captured rollout is the true-window one, on
    float *ro_graph_slab;          // this slab
    int last_n;                    // samples of the last gradient pass (grl_fnet_apply_grads normalises the loss sums with it)
};

namespace grl {

static FlatArgs base_args(grl_fnet *net, int n, const float *states, const float *hist, float *mu, float *sigma, float *vs, bool save,
                          const int32_t *nhist = nullptr, int wstride = 0) {
    FlatArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.S0 = net->cfg.static_size; a.D = net->cfg.temporal_size; a.T = net->cfg.rnn_length;
    a.A = net->cfg.num_actions; a.scale = net->cfg.scale; a.bound = net->cfg.mu_bound; a.states = states; a.hist = hist;
    a.mu = mu; a.sigma = sigma; a.vs = vs; a.ws = save ? net->ws : nullptr; a.nhist = nhist;
    a.ts = net->d_ts; a.ts_n = net->d_ts_n; a.wstride = wstride;
    return a;
}

static int launch_forward(grl_fnet *net, int n, const float *states, const float *hist, float *mu, float *sigma, float *vs, bool save,
                          const int32_t *nhist = nullptr, int wstride = 0) {
    FlatArgs a = base_args(net, n, states, hist, mu, sigma, vs, save, nhist, wstride);
    const int groups = (n + 63) / 64;
    if (wstride && !save) {
        // true windows, predictions only: the fast forward for distinct rows (net_flat_window.inc)
        if (net->cfg.temporal_size <= 4) hipLaunchKernelGGL(flat_forward_win_kernel<1>, dim3(groups), dim3(FNT), ff_lds_bytes(net->cfg.static_size), net->h->stream, a);
        else hipLaunchKernelGGL(flat_forward_win_kernel<9>, dim3(groups), dim3(FNT), ff_lds_bytes(net->cfg.static_size), net->h->stream, a);
        PAAC_HIP(net, hipGetLastError());
        return GRL_OK;
    }
    if (nhist && !wstride && net->cfg.static_size == net->cfg.temporal_size && net->fast_forward) {
        // synthesized window (the PAAC worker's: the current state repeated): the 2T + 5 stage form of net_flat_fast.inc
        if (save) hipLaunchKernelGGL(flat_forward_fast_kernel<true>, dim3(groups), dim3(FNT), ff_lds_bytes(net->cfg.static_size), net->h->stream, a);
        else hipLaunchKernelGGL(flat_forward_fast_kernel<false>, dim3(groups), dim3(FNT), ff_lds_bytes(net->cfg.static_size), net->h->stream, a);
        PAAC_HIP(net, hipGetLastError());
        return GRL_OK;
    }
    const size_t wbytes = (size_t)(net->cfg.temporal_size + FH) * 3 * FH * sizeof(float);
    static const int wlds_max_groups = getenv("GRL_FLAT_WLDS_GROUPS") ? atoi(getenv("GRL_FLAT_WLDS_GROUPS")) : 256;      // one workgroup per CU; measured (tools/bench_trade_sizes.py): 128 / 256 groups 7.6 -> 5.5 ms, 384 / 512 groups 8.5 -> 10.4 ms
    if (groups <= wlds_max_groups)
        hipLaunchKernelGGL(flat_forward_kernel<true>, dim3(groups), dim3(256), FLAT_LDS_BYTES + wbytes, net->h->stream, a, (int)FLAT_LDS_ROWS);
    else
        hipLaunchKernelGGL(flat_forward_kernel<false>, dim3(groups), dim3(256), FLAT_LDS_BYTES, net->h->stream, a, (int)FLAT_LDS_ROWS);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

// forward(save) + backward over n device-resident samples; grads <- gradient of the mean loss over THESE n samples
// resident: the workspace already holds this forward (the rollout that produced the samples kept its activations, and the
// parameters have not moved since): the pass starts at the backward
static int train_grads_device(grl_fnet *net, int n, const float *states, const float *hist, const float *actions, const float *adv,
                              const float *y, const int32_t *nhist = nullptr, bool resident = false, int wstride = 0) {
    hipStream_t st = net->h->stream;
    if (n > net->cfg.max_samples) return paac_fail(net, GRL_E_SIZE, "train: n exceeds max_samples of the net");
    int rc = GRL_OK;
    if (!resident) {
        net->ws_resident = 0;
        rc = launch_forward(net, n, states, hist, net->mu, net->sigma, net->vs, true, nhist, wstride);
    }
    if (rc) return rc;
    int groups = (n + 63) / 64;
    // true windows (wstride): the general forward and backward over the strided views; a fast backward for distinct rows does not exist
    const bool fast = nhist && !wstride && net->cfg.static_size == net->cfg.temporal_size && net->fast_forward && net->arg_slot >= 0;
    int blocks = groups < net->slab_blocks ? groups : net->slab_blocks;
    if (fast && blocks > 256) blocks = 256;      // the 16-wave form: one workgroup per CU (100 KB of LDS)
    if (!fast) PAAC_HIP(net, hipMemsetAsync(net->slab, 0, (size_t)blocks * net->off.total * 4, st));      // the fast backward clears its own
    PAAC_HIP(net, hipMemsetAsync(net->stats64, 0, 4 * sizeof(double), st));
    FlatArgs a = base_args(net, n, states, hist, net->mu, net->sigma, net->vs, true, nhist, wstride);
    a.actions = actions; a.adv = adv; a.y = y; a.inv_n = 1.0f / (float)n; a.slab = net->slab; a.stats64 = net->stats64;
    if (fast && net->arg_slot >= 0) {
        a.PT = net->paramsT;
        hipLaunchKernelGGL(flat_transpose_kernel, dim3(kFlatTransposed), dim3(256), 0, st, net->params, net->paramsT, net->off,
                           net->cfg.temporal_size, net->cfg.num_actions);
        // the stages of the fast backward are calls that read their arguments from the net's __constant__ slot (net_flat_fast.inc)
        PAAC_HIP(net, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_flat_args), &a, sizeof(FlatArgs), (size_t)net->arg_slot * sizeof(FlatArgs),
                                             hipMemcpyHostToDevice, st));
        (void)hipGetLastError();
        hipLaunchKernelGGL(flat_backward_fast_kernel, dim3(blocks), dim3(FNT), FB2_LDS_BYTES, st, net->arg_slot, n, net->cfg.rnn_length, a.ts, a.ts_n);
    } else {
        hipLaunchKernelGGL(flat_backward_kernel, dim3(blocks), dim3(256), FLAT_LDS_BYTES, st, a);
    }
    hipLaunchKernelGGL(flat_slab_reduce_kernel, dim3((unsigned)((net->off.total + 63) / 64)), dim3(1024), 0, st, net->slab, blocks,
                       net->off.total, net->grads);
    PAAC_HIP(net, hipGetLastError());
    net->last_n = n;
    return GRL_OK;
}

// global norm of grad_scale * grads, clip factor, loss statistics of the last gradient pass; then (apply_update) Adam
static int train_apply_device(grl_fnet *net, float lr, int apply_update, float grad_scale, float *stats_host) {
    hipStream_t st = net->h->stream;
    const int n = net->last_n;
    hipLaunchKernelGGL(flat_sumsq_kernel, dim3(kSumsqBlocks), dim3(256), 0, st, net->grads, net->off.total, net->stats64 + 4);
    hipLaunchKernelGGL(flat_finalize_kernel, dim3(1), dim3(64), 0, st, net->stats64 + 4, net->stats64, 1.0f / (float)n,
                       1.0f / ((float)n * (float)net->cfg.num_actions), net->cfg.clip_norm, grad_scale, net->stats);
    if (apply_update) {
        net->ws_resident = 0;      // the parameters move
        net->adam_t += 1;
        hipLaunchKernelGGL(paac_adam_kernel<>, dim3((unsigned)((net->off.total + 255) / 256)), dim3(256), 0, st, net->params, net->grads,
                           net->adam_m, net->adam_v, net->off.total, net->stats, adam_lr_t(lr, net->adam_t));
    }
    PAAC_HIP(net, hipGetLastError());
    PAAC_HIP(net, hipStreamSynchronize(st));
    paac_allreduce_account(net);
    return paac_read_stats(net, stats_host);
}

// gradient pass [+ all-reduce over ranks if a communicator is attached and the parameters are to be updated] + clip + Adam
static int train_device(grl_fnet *net, int n, const float *states, const float *hist, const float *actions, const float *adv, const float *y,
                        float lr, int apply_update, float *stats_host, const int32_t *nhist = nullptr, bool resident = false, int wstride = 0) {
    int rc = train_grads_device(net, n, states, hist, actions, adv, y, nhist, resident, wstride);
    if (rc) return rc;
    float grad_scale = 1.0f;
    if (apply_update && (rc = paac_allreduce_grads(net, net->grads, nullptr, &grad_scale))) return rc;
    return train_apply_device(net, lr, apply_update, grad_scale, stats_host);
}

// ---- true window (net_flat_window.inc): the state the net keeps between calls
// the slab for rollouts of T steps; ro_states points behind its rnn - 1 leading slices
static int window_ensure_slab(grl_fnet *net, int T) {
    const size_t slice = (size_t)net->h->E * net->cfg.static_size, lead = (size_t)net->cfg.rnn_length - 1;
    int rc = GRL_OK;
    if (!net->w_len) {
        if ((rc = paac_alloc(net, &net->w_len, net->h->E))) return rc;
        if ((rc = paac_alloc(net, &net->w_elapsed, net->h->E))) return rc;
        if ((rc = paac_alloc(net, &net->w_episode, net->h->E))) return rc;
        net->w_restart_all = 1;
    }
    if (!net->ro_slab || net->slab_T < T) {
        // an older slab stays allocated until the net is destroyed: w_src may still point into it
        if ((rc = paac_alloc(net, &net->ro_slab, (lead + (size_t)T + 1) * slice))) return rc;
        net->slab_T = T;
    }
    net->ro_states = net->ro_slab + lead * slice;
    return GRL_OK;
}

// before a forward on the handle's current observation: the rows behind it move to the front of the slab (once), and windows
// restart for every env the host reset or stepped since the net last looked (or for all of them)
static int window_enter(grl_fnet *net) {
    grl_handle *h = net->h;
    const int E = h->E, lead = net->cfg.rnn_length - 1;
    const long slice = (long)E * net->cfg.static_size;
    hipStream_t st = h->stream;
    const int all = (net->w_restart_all || !net->w_have) ? 1 : 0;
    if (!all && lead > 0 && net->w_src && net->w_src != net->ro_slab)
        hipLaunchKernelGGL(flat_window_carry_kernel, dim3((unsigned)((slice + 255) / 256)), dim3(256), 0, st, net->w_src, net->ro_slab, lead, slice);
    net->w_src = net->ro_slab;
    net->w_valid = 0;
    hipLaunchKernelGGL(flat_window_detect_kernel, dim3((E + 255) / 256), dim3(256), 0, st, net->w_len, (const int32_t *)h->elapsed,
                       (const int32_t *)h->episode, (const int32_t *)net->w_elapsed, (const int32_t *)net->w_episode, E, all);
    PAAC_HIP(net, hipGetLastError());
    net->w_restart_all = 0;
    return GRL_OK;
}

// behind a rollout of T steps: what the net has seen of every env, and where the next rollout's leading rows lie
static int window_leave(grl_fnet *net, int T) {
    grl_handle *h = net->h;
    const long slice = (long)h->E * net->cfg.static_size;
    PAAC_HIP(net, hipMemcpyAsync(net->w_elapsed, h->elapsed, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
    PAAC_HIP(net, hipMemcpyAsync(net->w_episode, h->episode, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
    net->w_src = net->ro_states + ((long)T - (net->cfg.rnn_length - 1)) * slice;
    net->w_have = 1;
    net->w_valid = 1;
    return GRL_OK;
}

// the T-step actor loop as stream operations (captured into a graph by grl_fnet_rollout)
static int enqueue_rollout(grl_fnet *net, int T) {
    grl_handle *h = net->h;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E, R = net->cfg.rnn_length, S0 = net->cfg.static_size, A = net->cfg.num_actions;
    hipStream_t st = h->stream;
    const float *obs = solow ? h->so.obs : h->tr.obs;
    int rc;
    for (int t = 0; t < T; ++t) {
        // states[t] = shared_states, histories[t] = shared_histories (paac.py:132-133).  For TradeAR1 the window is
        // kept as (state, #rows): the worker's history is min(n, rnn) copies of the current state (quirk Q11)
        PAAC_HIP(net, hipMemcpyAsync(net->ro_states + (size_t)t * E * S0, obs, (size_t)E * S0 * 4, hipMemcpyDeviceToDevice, st));
        // the window is kept as (state, #rows) for both envs -- the worker's history is min(n, rnn) copies of the current state
        // (quirk Q11); Solow's dense (E, rnn, 2) form is recorded too (grl_fnet_read_rollout "histories")
        const int32_t *nh = solow ? h->so.nhist : h->tr.nhist;
        if (net->true_window) {
            // the window: the rows of the slab that end at states[t] (w_len of them per env)
            PAAC_HIP(net, hipMemcpyAsync(net->ro_nhist + (size_t)t * E, net->w_len, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
            rc = launch_forward(net, E, net->ro_states + (size_t)t * E * S0, nullptr, net->mu, net->sigma, net->ro_val + (size_t)t * E, false, net->w_len, E);
            if (rc) return rc;
        } else {
        if (solow) PAAC_HIP(net, hipMemcpyAsync(net->ro_hist + (size_t)t * E * R * 2, h->so.history, (size_t)E * R * 8, hipMemcpyDeviceToDevice, st));
        PAAC_HIP(net, hipMemcpyAsync(net->ro_nhist + (size_t)t * E, nh, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
        rc = launch_forward(net, E, obs, nullptr, net->mu, net->sigma, net->ro_val + (size_t)t * E, false, nh);
        if (rc) return rc;
        }
        hipLaunchKernelGGL(flat_sample_kernel, dim3((E * A + 255) / 256), dim3(256), 0, st, net->mu, net->sigma, E, A, h->cfg.seed,
                           (uint32_t)h->cfg.env_id_offset, (const uint32_t *)net->d_counter, (uint32_t)t, h->cfg.env_kind, net->greedy,
                           net->ro_act + (size_t)t * E * A, net->ro_envact);
        rc = solow ? solow_launch_step(h, net->ro_envact) : trade_launch_step(h, net->ro_envact);
        if (rc) return paac_fail(net, rc, h->err);
        if ((rc = episodes_launch_account(h))) return paac_fail(net, rc, h->err);      // R6 (paac.py:142-157), when enabled on the handle
        PAAC_HIP(net, hipMemcpyAsync(net->ro_rew + (size_t)t * E, h->reward, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(flat_mask_kernel, dim3((E + 255) / 256), dim3(256), 0, st, h->done, E, net->ro_mask + (size_t)t * E);
        if (net->true_window)
            hipLaunchKernelGGL(flat_window_step_kernel, dim3((E + 255) / 256), dim3(256), 0, st, net->w_len, (const uint8_t *)h->done, E, R);
    }
    if (net->true_window) {      // the bootstrap observation is slice T of the slab: the window behind the last step
        PAAC_HIP(net, hipMemcpyAsync(net->ro_states + (size_t)T * E * S0, obs, (size_t)E * S0 * 4, hipMemcpyDeviceToDevice, st));
        rc = launch_forward(net, E, net->ro_states + (size_t)T * E * S0, nullptr, net->mu, net->sigma, net->ro_boot, false, net->w_len, E);
    } else {
        rc = launch_forward(net, E, obs, nullptr, net->mu, net->sigma, net->ro_boot, false, solow ? h->so.nhist : h->tr.nhist);
    }
    if (rc) return rc;
    // rewards clipped to [-2, 2] (paac.py:145), masked n-step return (paac.py:167-172), adv / scale (paac.py:177)
    // gae_lambda < 1: the A3C worker's GAE on the raw rewards (a3c/worker.py:232-294)
    const bool gae = net->cfg.gae_lambda < 1.0f;
    if ((rc = launch_returns(h, net->ro_rew, net->ro_val, net->ro_mask, net->ro_boot, T, E, net->cfg.gamma, gae ? net->cfg.gae_lambda : 1.0f,
                             net->cfg.scale, gae ? 0.f : -2.f, gae ? 0.f : 2.f, net->ro_y, net->ro_adv)))
        return paac_fail(net, rc, h->err);
    return GRL_OK;
}

// the T-step actor loop as ONE kernel: a workgroup owns 64 envs for the whole rollout (net_flat_rollout.inc).  Returns
// GRL_E_SIZE when the rollout's LDS footprint does not fit a CU (the caller then takes the graph path).
// slots of g_flat_args: one per live net of the process (a net that finds none free keeps the graph path)
static std::mutex g_slot_mu;
static bool g_slot_used[kFlatArgSlots];
static int flat_slot_take() {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    for (int i = 0; i < kFlatArgSlots; ++i)
        if (!g_slot_used[i]) { g_slot_used[i] = true; return i; }
    return -1;
}
static void flat_slot_release(int i) {
    if (i < 0) return;
    std::lock_guard<std::mutex> lk(g_slot_mu);
    g_slot_used[i] = false;
}

static int launch_persistent_rollout(grl_fnet *net, int T) {
    grl_handle *h = net->h;
    if (net->arg_slot < 0) return GRL_E_SIZE;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    RolloutArgs R{};
    R.f = base_args(net, h->E, nullptr, nullptr, nullptr, nullptr, nullptr, false);
    const bool tw = net->true_window != 0;
    const bool keep = net->keep_activations != 0 && !tw;      // true window: accepted and ignored, the gradient step recomputes
    if (keep) R.f.ws = net->ws;
    R.steps = T; R.env_kind = h->cfg.env_kind; R.slot = net->arg_slot;
    const int n_assets = solow ? 0 : h->cfg.n_assets;
    size_t lds_bytes = (size_t)rollout_lds_floats(net->cfg.static_size, T, n_assets, &R) * sizeof(float);
    if (tw) {      // one more row of ints behind everything: the window's rows per env; the forward reads the windows from the slab
        R.off_wl = (int)(lds_bytes / sizeof(float));
        lds_bytes += 64 * sizeof(float);
        R.wlen = net->w_len; R.f.states = net->ro_states; R.f.wstride = h->E;
    }
    if (lds_bytes > 160 * 1024) return GRL_E_SIZE;
    // envs per workgroup: a workgroup has a CU to itself (LDS), and a group's chain of stages is as long for 16 envs as for 64 with
    // fewer tiles per stage -- so the smallest group that still gives every CU at most one workgroup (GRL_FLAT_GROUP = 64 / 32 / 16
    // fixes it).  Measured at the end of round 5 (tools/flat_group_sweep.py, ms per 20-step rollout, G = 64 / 32 / 16): TradeAR1-16
    // 1 024 envs 1.74 / 1.25 / 1.16, 4 096: 1.76 / 1.25 / 1.17, 8 192: 1.76 / 1.26 / 2.30, 16 384: 1.78 / 2.48 / 4.55; Solow 4 096:
    // 0.79 / 0.51 / 0.48, 8 192: 0.80 / 0.51 / 0.91.  (While every forward call still moved 44 callee-saved registers through
    // scratch, 256 workgroups at once were slower than 128 and groups of 16 paid only up to 1 024 envs.)
    int G = net->ro_group;
    if (!G) G = h->E <= 16 * 256 ? 16 : (h->E <= 32 * 256 ? 32 : 64);
    R.gs = G;
    typedef void (*RoKernel)(int);
    static const RoKernel kernels[2][3] = {{flat_rollout_kernel<16, false>, flat_rollout_kernel<32, false>, flat_rollout_kernel<64, false>},
                                           {flat_rollout_kernel<16, true>, flat_rollout_kernel<32, true>, flat_rollout_kernel<64, true>}};
    static const RoKernel win_kernels[3] = {flat_rollout_win_kernel<16>, flat_rollout_win_kernel<32>, flat_rollout_win_kernel<64>};
    const int gi = G == 16 ? 0 : (G == 32 ? 1 : 2);
    const RoKernel kern_fn = tw ? win_kernels[gi] : kernels[keep ? 1 : 0][gi];
    const void *kern = (const void *)kern_fn;
    // the attribute belongs to the kernel (per device), not to the net: every net raises it to the CU's whole LDS, so that no net's
    // smaller rollout lowers it under another net's larger one
    char &attr_set = tw ? net->ro_win_attr_set[gi] : net->ro_attr_set[keep ? 1 : 0][gi];
    if (!attr_set) {
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            return GRL_E_SIZE;
        }
        attr_set = 1;
    }
    if (solow) {
        R.so = solow_params(h);
        R.needs_tape = (!(h->cfg.flags & GRL_F_RESET_FROM_SNAPSHOT) && h->cfg.max_episode_steps > 0) ? 1 : 0;
        R.obs0 = h->so.obs;
    } else {
        R.tr = trade_params(h);
        R.obs0 = h->tr.obs;
    }
    R.ro_states = net->ro_states; R.ro_hist = net->ro_hist; R.ro_act = net->ro_act; R.ro_val = net->ro_val; R.ro_rew = net->ro_rew;
    R.ro_mask = net->ro_mask; R.ro_y = net->ro_y; R.ro_adv = net->ro_adv; R.ro_boot = net->ro_boot; R.ro_nhist = net->ro_nhist;
    R.counter_base = net->d_counter; R.seed = h->cfg.seed; R.env_off = (uint32_t)h->cfg.env_id_offset;
    const bool gae = net->cfg.gae_lambda < 1.0f;
    R.gamma = net->cfg.gamma; R.lam = gae ? net->cfg.gae_lambda : 1.0f; R.clip_lo = gae ? 0.f : -2.f; R.clip_hi = gae ? 0.f : 2.f;
    R.ep_total = h->ep_total; R.ep_len = h->ep_len; R.ep_steps = h->ep_steps; R.ep_rec = h->ep_rec; R.ep_count = h->ep_count;
    R.ep_cap = h->ep_capacity;
    hipStream_t st = h->stream;
    R.ts = net->d_ts; R.ts_n = net->d_ts_n; R.greedy = net->greedy;
    if (net->d_ts_n) PAAC_HIP(net, hipMemsetAsync(net->d_ts_n, 0, sizeof(int), st));
    PAAC_HIP(net, hipMemsetAsync(h->done_count, 0, sizeof(int32_t), st));      // the last step's done list is built inside the kernel
    PAAC_HIP(net, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ro_args), &R, sizeof(RolloutArgs), (size_t)net->arg_slot * sizeof(RolloutArgs),
                                         hipMemcpyHostToDevice, st));      // pageable source: staged before the call returns
    PAAC_HIP(net, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_flat_args), &R.f, sizeof(FlatArgs), (size_t)net->arg_slot * sizeof(FlatArgs),
                                         hipMemcpyHostToDevice, st));
    (void)hipGetLastError();      // the symbol lookup may probe other ordinals and leave a stale error on this thread
    const dim3 grid((h->E + G - 1) / G);
    hipLaunchKernelGGL(kern_fn, grid, dim3(FNT), lds_bytes, st, net->arg_slot);
    PAAC_HIP(net, hipGetLastError());
    net->ws_resident = keep ? 1 : 0;
    return GRL_OK;
}

// the result and trace buffers of grl_fnet_eval for `steps` traced steps
static int ensure_eval_buffers(grl_fnet *net, int steps) {
    const size_t E = net->h->E;
    int rc = GRL_OK;
    if (!net->ev_total) {
        if ((rc = paac_alloc(net, &net->ev_total, E))) return rc;
        if ((rc = paac_alloc(net, &net->ev_len, E))) return rc;
        if ((rc = paac_alloc(net, &net->ev_fin, E))) return rc;
    }
    if (steps <= net->ev_trace_cap) return GRL_OK;
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ev_allocs) hipFree(p);
    net->ev_allocs.clear();
    net->ev_trace_cap = -1;
    const size_t SE = (size_t)steps * E, S0 = net->cfg.static_size, A = net->cfg.num_actions;
    hipStream_t st = net->h->stream;
    auto Al = [&](auto **p, size_t cnt) {
        if (rc != GRL_OK) return;
        cnt = cnt ? cnt : 1;
        hipError_t e = hipMalloc((void **)p, cnt * sizeof(**p));
        if (e == hipSuccess) { net->ev_allocs.push_back(*p); e = hipMemsetAsync(*p, 0, cnt * sizeof(**p), st); }
        if (e != hipSuccess) rc = paac_fail(net, GRL_E_HIP, std::string("eval trace buffers: ") + hipGetErrorString(e));
    };
    Al(&net->ev_states, SE * S0); Al(&net->ev_nhist, SE); Al(&net->ev_mu, SE * A); Al(&net->ev_sigma, SE * A); Al(&net->ev_raw, SE * A);
    Al(&net->ev_act, SE * A); Al(&net->ev_val, SE); Al(&net->ev_rew, SE); Al(&net->ev_done, SE);
    if (rc == GRL_OK) net->ev_trace_cap = steps;
    return rc;
}

// whole episodes of every env as ONE kernel (net_flat_eval.inc)
static int launch_eval(grl_fnet *net, int max_steps, int trace_steps, int greedy) {
    grl_handle *h = net->h;
    if (net->arg_slot < 0) return paac_fail(net, GRL_E_STATE, "grl_fnet_eval: no constant-memory argument slot is free for this net");
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    RolloutArgs R{};
    R.f = base_args(net, h->E, nullptr, nullptr, nullptr, nullptr, nullptr, false);
    R.f.ts = nullptr; R.f.ts_n = nullptr;
    R.steps = 0; R.env_kind = h->cfg.env_kind; R.slot = net->arg_slot;
    int live_off = 0;
    const bool tw = net->true_window != 0;
    size_t lds_bytes = (size_t)eval_lds_floats(net->cfg.static_size, solow ? 0 : h->cfg.n_assets, &R, &live_off) * sizeof(float);
    if (tw) {      // the window's rows per env behind the live word; the last rnn states of every env in a ring of time slices
        R.off_wl = (int)(lds_bytes / sizeof(float));
        lds_bytes += 64 * sizeof(float);
        if (!net->ev_ring) {
            int rc = paac_alloc(net, &net->ev_ring, (size_t)net->cfg.rnn_length * h->E * net->cfg.static_size);
            if (rc) return rc;
        }
        R.f.states = net->ev_ring; R.f.wstride = h->E; R.f.wring = net->cfg.rnn_length;
    }
    if (lds_bytes > 160 * 1024) return paac_fail(net, GRL_E_SIZE, "grl_fnet_eval: the evaluation's LDS rows do not fit a CU");
    int G = net->ro_group;      // the rule of launch_persistent_rollout
    if (!G) G = h->E <= 16 * 256 ? 16 : (h->E <= 32 * 256 ? 32 : 64);
    R.gs = G;
    typedef void (*EvKernel)(int, int);
    static const EvKernel quirk_kernels[3] = {flat_eval_kernel<16>, flat_eval_kernel<32>, flat_eval_kernel<64>};
    static const EvKernel win_kernels[3] = {flat_eval_win_kernel<16>, flat_eval_win_kernel<32>, flat_eval_win_kernel<64>};
    const EvKernel *kernels = tw ? win_kernels : quirk_kernels;
    const int gi = G == 16 ? 0 : (G == 32 ? 1 : 2);
    char &ev_attr = tw ? net->ev_win_attr_set[gi] : net->ev_attr_set[gi];
    if (!ev_attr) {
        PAAC_HIP(net, hipFuncSetAttribute((const void *)kernels[gi], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ev_attr = 1;
    }
    if (solow) { R.so = solow_params(h); R.obs0 = h->so.obs; }
    else { R.tr = trade_params(h); R.obs0 = h->tr.obs; }
    R.counter_base = net->d_counter; R.seed = h->cfg.seed; R.env_off = (uint32_t)h->cfg.env_id_offset;
    R.greedy = greedy ? 1 : 0;
    R.ev.max_steps = max_steps; R.ev.trace_steps = trace_steps;
    R.ev.total = net->ev_total; R.ev.length = net->ev_len; R.ev.finished = net->ev_fin;
    R.ev.states = net->ev_states; R.ev.nhist = net->ev_nhist; R.ev.mu = net->ev_mu; R.ev.sigma = net->ev_sigma; R.ev.raw = net->ev_raw;
    R.ev.act = net->ev_act; R.ev.val = net->ev_val; R.ev.rew = net->ev_rew; R.ev.done = net->ev_done;
    hipStream_t st = h->stream;
    PAAC_HIP(net, hipMemsetD32Async((hipDeviceptr_t)net->d_counter, (int)(uint32_t)net->act_counter, 1, st));
    PAAC_HIP(net, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ro_args), &R, sizeof(RolloutArgs), (size_t)net->arg_slot * sizeof(RolloutArgs),
                                         hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_flat_args), &R.f, sizeof(FlatArgs), (size_t)net->arg_slot * sizeof(FlatArgs),
                                         hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernels[gi], dim3((h->E + G - 1) / G), dim3(FNT), lds_bytes, st, net->arg_slot, live_off);
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_fnet_config_default(grl_fnet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_fnet_config);
    cfg->static_size = 2; cfg->temporal_size = 2; cfg->rnn_length = 5; cfg->num_actions = 1;     // train_paac_solow.py:96-129
    cfg->rnn_hidden = 32; cfg->static_hidden = 32; cfg->max_samples = 4096 * 20;
    cfg->scale = 100.f; cfg->clip_norm = 40.f; cfg->gamma = 0.99f; cfg->mu_bound = 5.f; cfg->gae_lambda = 1.f;
    return GRL_OK;
}

int grl_fnet_create(grl_handle *h, const grl_fnet_config *cfg, grl_fnet **out) {
    if (!h || !cfg || !out) return GRL_E_INVALID;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(grl_fnet_config)) return fail(h, GRL_E_INVALID, "grl_fnet_create: config size mismatch");
    if (cfg->rnn_hidden != FH || cfg->static_hidden != FH) return fail(h, GRL_E_INVALID, "grl_fnet_create: hidden sizes must be 32 (the reference defaults)");
    if (cfg->temporal_size < 1 || cfg->temporal_size > MAXD || cfg->static_size < 1 || cfg->static_size > MAXS0 || cfg->num_actions < 1 ||
        cfg->num_actions > MAXA || cfg->rnn_length < 1 || cfg->rnn_length > 32 || cfg->max_samples < 1)
        return fail(h, GRL_E_INVALID, "grl_fnet_create: size out of range");
    if (!(cfg->gae_lambda > 0.f && cfg->gae_lambda <= 1.f)) return fail(h, GRL_E_INVALID, "grl_fnet_create: gae_lambda must be in (0, 1]");
    hipSetDevice(h->cfg.device_id);
    grl_fnet *n = new grl_fnet();
    n->h = h; n->cfg = *cfg;
    n->off = make_offsets(cfg->temporal_size, cfg->static_size, cfg->num_actions); n->num_params = n->off.total;
    n->wso = ws_offsets(cfg->rnn_length, cfg->num_actions);
    n->slab_blocks = 512;      // two workgroups per CU (LDS 75 KB each)
    size_t ms = cfg->max_samples;
    const int A = cfg->num_actions, S0 = cfg->static_size, D = cfg->temporal_size, T = cfg->rnn_length;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = paac_alloc(n, p, cnt); };
    Al(&n->params, n->off.total); Al(&n->paramsT, n->off.total); Al(&n->grads, n->off.total); Al(&n->adam_m, n->off.total); Al(&n->adam_v, n->off.total);
    Al(&n->ws, (ms + 63) / 64 * 64 * n->wso.total); Al(&n->slab, (size_t)n->slab_blocks * n->off.total); Al(&n->stats, 8);
    Al(&n->d_states, ms * S0); Al(&n->d_hist, ms * T * D); Al(&n->d_act, ms * A); Al(&n->d_adv, ms); Al(&n->d_y, ms);
    Al(&n->mu, ms * A); Al(&n->sigma, ms * A); Al(&n->vs, ms);
    if (rc == GRL_OK) rc = paac_alloc(n, &n->stats64, 4 + kSumsqBlocks);      // loss sums (2 used of 4), then the squares' partial sums
    if (rc == GRL_OK) rc = paac_alloc(n, &n->d_counter, 4);
    n->ro_graph = nullptr; n->ro_graph_T = 0; n->ro_graph_ep = false; n->ro_graph_greedy = 0; n->greedy = 0;
    n->ev_total = nullptr; n->ev_trace = 0; n->ev_trace_cap = -1; n->ev_played = -2; memset(n->ev_attr_set, 0, sizeof(n->ev_attr_set));
    {   // GRL_FLAT_ROLLOUT=graph keeps the launch-per-stage rollout (captured into a hipGraph) for A/B and for the equality tests
        const char *e = getenv("GRL_FLAT_ROLLOUT");
        n->ro_persistent = (e && strcmp(e, "graph") == 0) ? 0 : 1;
        memset(n->ro_attr_set, 0, sizeof(n->ro_attr_set)); n->d_ts = nullptr; n->d_ts_n = nullptr;
        n->keep_activations = 0; n->ws_resident = 0;
        const char *g = getenv("GRL_FLAT_GROUP");
        const int gv = g ? atoi(g) : 0;
        n->ro_group = (gv == 16 || gv == 32 || gv == 64) ? gv : 0;
        n->arg_slot = flat_slot_take();
        const char *f = getenv("GRL_FLAT_FORWARD");
        n->fast_forward = (f && strcmp(f, "layers") == 0) ? 0 : 1;
    }
    n->true_window = 0; n->ro_slab = nullptr; n->slab_T = 0; n->w_len = n->w_elapsed = n->w_episode = nullptr; n->w_src = nullptr;
    n->w_restart_all = 1; n->w_have = 0; n->w_valid = 0; n->ev_ring = nullptr; n->ro_graph_tw = 0;
    memset(n->ro_win_attr_set, 0, sizeof(n->ro_win_attr_set)); memset(n->ev_win_attr_set, 0, sizeof(n->ev_win_attr_set));
    n->last_n = 0;
    hipError_t e = hipSuccess;
    if (rc == GRL_OK) e = hipFuncSetAttribute((const void *)flat_forward_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLAT_LDS_BYTES);
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_forward_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(FLAT_LDS_BYTES + (size_t)(MAXD + FH) * 3 * FH * sizeof(float)));
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLAT_LDS_BYTES);
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_forward_fast_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ff_lds_bytes(MAXS0));
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_forward_fast_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ff_lds_bytes(MAXS0));
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_forward_win_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ff_lds_bytes(MAXS0));
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_forward_win_kernel<9>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ff_lds_bytes(MAXS0));
    if (rc == GRL_OK && e == hipSuccess)
        e = hipFuncSetAttribute((const void *)flat_backward_fast_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB2_LDS_BYTES);
    if (rc == GRL_OK && e != hipSuccess) rc = paac_fail(n, GRL_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    if (rc != GRL_OK) {
        fail(h, rc, "grl_fnet_create: " + n->err);
        grl_fnet_destroy(n);
        return rc;
    }
    hipStreamSynchronize(h->stream);
    *out = n;
    return GRL_OK;
}

int grl_fnet_destroy(grl_fnet *n) {
    if (!n) return GRL_OK;
    grl_sync_for_destroy(n->h);      // the handle may have been destroyed first (finaliser order of a host binding)
    if (n->ro_graph) (void)hipGraphExecDestroy(n->ro_graph);
    paac_comm_release(n);
    flat_slot_release(n->arg_slot);
    paac_free(n);
    for (void *p : n->ev_allocs) hipFree(p);
    delete n;
    return GRL_OK;
}

const char *grl_fnet_last_error(const grl_fnet *n) { return paac_last_error(n); }
int64_t grl_fnet_num_params(const grl_fnet *n) { return paac_num_params(n); }

int grl_fnet_set_params(grl_fnet *n, const float *host, int64_t cnt) {
    if (n) n->ws_resident = 0;
    return paac_copy_flat(n, nullptr, n ? n->params : nullptr, (float *)host, cnt, true);
}

int grl_fnet_set_keep_activations(grl_fnet *net, int32_t on) {
    if (!net) return GRL_E_INVALID;
    net->keep_activations = on ? 1 : 0;
    return GRL_OK;
}
int grl_fnet_get_params(grl_fnet *n, float *host, int64_t cnt) { return paac_copy_flat(n, nullptr, n ? n->params : nullptr, host, cnt, false); }
int grl_fnet_get_grads(grl_fnet *n, float *host, int64_t cnt) { return paac_copy_flat(n, nullptr, n ? n->grads : nullptr, host, cnt, false); }

int grl_fnet_get_optimizer_state(grl_fnet *n, float *m_host, float *v_host, int64_t cnt, int64_t *step_out) {
    return paac_get_optimizer_state(n, m_host, v_host, cnt, step_out);
}
int grl_fnet_set_optimizer_state(grl_fnet *n, const float *m_host, const float *v_host, int64_t cnt, int64_t step) {
    return paac_set_optimizer_state(n, nullptr, m_host, v_host, cnt, step);
}

int grl_fnet_get_action_counter(grl_fnet *net, uint64_t *out) { return paac_get_action_counter(net, out); }
int grl_fnet_set_action_counter(grl_fnet *net, uint64_t value) { return paac_set_action_counter(net, value); }

static int fdownload(grl_fnet *net, int n, float *mu, float *sigma, float *vs) {
    const int A = net->cfg.num_actions;
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    if (mu) PAAC_HIP(net, hipMemcpy(mu, net->mu, (size_t)n * A * 4, hipMemcpyDeviceToHost));
    if (sigma) PAAC_HIP(net, hipMemcpy(sigma, net->sigma, (size_t)n * A * 4, hipMemcpyDeviceToHost));
    if (vs) PAAC_HIP(net, hipMemcpy(vs, net->vs, (size_t)n * 4, hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_fnet_predict(grl_fnet *net, int32_t n, const float *states, const float *history, float *mu, float *sigma, float *vs) {
    if (!net || n <= 0 || !states || !history) return paac_fail(net, GRL_E_INVALID, "grl_fnet_predict: bad argument");
    if (n > net->cfg.max_samples) return paac_fail(net, GRL_E_SIZE, "grl_fnet_predict: n exceeds max_samples");
    hipSetDevice(net->h->cfg.device_id);
    const grl_fnet_config &c = net->cfg;
    hipStream_t st = net->h->stream;
    PAAC_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * c.static_size * 4, hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyAsync(net->d_hist, history, (size_t)n * c.rnn_length * c.temporal_size * 4, hipMemcpyHostToDevice, st));
    int rc = launch_forward(net, n, net->d_states, net->d_hist, net->mu, net->sigma, net->vs, false);
    if (rc) return rc;
    return fdownload(net, n, mu, sigma, vs);
}

static int check_env(grl_fnet *net) {
    grl_handle *h = net->h;
    if (h->cfg.env_kind == GRL_ENV_SOLOW) {
        if (net->cfg.static_size != 2 || net->cfg.temporal_size != 2 || net->cfg.rnn_length != h->cfg.rnn_length || net->cfg.num_actions != 1)
            return paac_fail(net, GRL_E_INVALID, "a Solow handle needs a net with static=temporal=2, num_actions=1 and the handle's rnn_length");
    } else if (h->cfg.env_kind == GRL_ENV_TRADE) {
        const int S = 1 + 2 * h->cfg.n_assets;      // INPUT_SIZE = TEMPORAL_SIZE = 1+2n, NUM_ACTIONS = n (train_trade.py:38-40)
        if (net->cfg.static_size != S || net->cfg.temporal_size != S || net->cfg.num_actions != h->cfg.n_assets ||
            net->cfg.rnn_length != h->cfg.rnn_length)
            return paac_fail(net, GRL_E_INVALID, "a TradeAR1 handle needs a net with static=temporal=1+2n, num_actions=n and the handle's rnn_length");
    } else {
        return paac_fail(net, GRL_E_INVALID, "this call needs a Solow or TradeAR1 handle");
    }
    if (h->E > net->cfg.max_samples) return paac_fail(net, GRL_E_SIZE, "num_envs exceeds max_samples of the net");
    return GRL_OK;
}

int grl_fnet_predict_env(grl_fnet *net, float *mu, float *sigma, float *vs) {
    if (!net) return GRL_E_INVALID;
    hipSetDevice(net->h->cfg.device_id);
    int rc = check_env(net);
    if (rc) return rc;
    grl_handle *h = net->h;
    if (net->true_window) {
        // the window the next rollout's first step would see: the rows behind it are carried forward now (the slab no longer
        // holds the last rollout: grl_fnet_train_rollout and grl_fnet_read_windows need a new one)
        const float *obs = h->cfg.env_kind == GRL_ENV_SOLOW ? h->so.obs : h->tr.obs;
        if ((rc = window_ensure_slab(net, net->T > 0 ? net->T : 1))) return rc;
        if ((rc = window_enter(net))) return rc;
        PAAC_HIP(net, hipMemcpyAsync(net->ro_states, obs, (size_t)h->E * net->cfg.static_size * 4, hipMemcpyDeviceToDevice, h->stream));
        if ((rc = launch_forward(net, h->E, net->ro_states, nullptr, net->mu, net->sigma, net->vs, false, net->w_len, h->E))) return rc;
        return fdownload(net, h->E, mu, sigma, vs);
    }
    if (h->cfg.env_kind == GRL_ENV_SOLOW) rc = launch_forward(net, h->E, h->so.obs, nullptr, net->mu, net->sigma, net->vs, false, h->so.nhist);
    else rc = launch_forward(net, h->E, h->tr.obs, nullptr, net->mu, net->sigma, net->vs, false, h->tr.nhist);
    if (rc) return rc;
    return fdownload(net, h->E, mu, sigma, vs);
}

int grl_fnet_train(grl_fnet *net, int32_t n, const float *states, const float *history, const float *actions, const float *advantages,
                   const float *critic_target, float lr, int32_t apply_update, float *stats_host) {
    if (!net || n <= 0 || !states || !history || !actions || !advantages || !critic_target) return paac_fail(net, GRL_E_INVALID, "grl_fnet_train: bad argument");
    if (n > net->cfg.max_samples) return paac_fail(net, GRL_E_SIZE, "grl_fnet_train: n exceeds max_samples");
    hipSetDevice(net->h->cfg.device_id);
    const grl_fnet_config &c = net->cfg;
    hipStream_t st = net->h->stream;
    PAAC_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * c.static_size * 4, hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyAsync(net->d_hist, history, (size_t)n * c.rnn_length * c.temporal_size * 4, hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyAsync(net->d_act, actions, (size_t)n * c.num_actions * 4, hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyAsync(net->d_adv, advantages, (size_t)n * 4, hipMemcpyHostToDevice, st));
    PAAC_HIP(net, hipMemcpyAsync(net->d_y, critic_target, (size_t)n * 4, hipMemcpyHostToDevice, st));
    return train_device(net, n, net->d_states, net->d_hist, net->d_act, net->d_adv, net->d_y, lr, apply_update, stats_host);
}

int grl_fnet_rollout(grl_fnet *net, int32_t T) {
    if (!net || T <= 0 || T > 1024) return paac_fail(net, GRL_E_INVALID, "grl_fnet_rollout: bad argument");
    hipSetDevice(net->h->cfg.device_id);
    int rc = check_env(net);
    if (rc) return rc;
    grl_handle *h = net->h;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E, R = net->cfg.rnn_length, S0 = net->cfg.static_size, A = net->cfg.num_actions;
    if ((long)T * E > net->cfg.max_samples) return paac_fail(net, GRL_E_SIZE, "grl_fnet_rollout: T*num_envs exceeds max_samples");
    const bool tw = net->true_window != 0;
    if (!net->ro_act || net->T < T) {
        auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = paac_alloc(net, p, cnt); };
        if (!tw) Al(&net->ro_states, (size_t)T * E * S0);      // true window: the states live in the slab
        Al(&net->ro_act, (size_t)T * E * A);
        Al(&net->ro_envact, (size_t)E * A); Al(&net->ro_val, (size_t)T * E); Al(&net->ro_rew, (size_t)T * E); Al(&net->ro_mask, (size_t)T * E);
        Al(&net->ro_y, (size_t)T * E); Al(&net->ro_adv, (size_t)T * E); Al(&net->ro_boot, E);
        if (solow) Al(&net->ro_hist, (size_t)T * E * R * 2);
        if (rc == GRL_OK) rc = paac_alloc(net, &net->ro_nhist, (size_t)T * E);
        if (rc) return rc;
    }
    if (tw) {
        if ((rc = window_ensure_slab(net, T))) return rc;
        if ((rc = window_enter(net))) return rc;
    }
    net->T = T;
    net->ws_resident = 0;      // set again by a persistent rollout that keeps its activations
    hipStream_t st = h->stream;
    // draw counter of step t = act_counter + t, read by the sample kernel from device memory
    PAAC_HIP(net, hipMemsetD32Async((hipDeviceptr_t)net->d_counter, (int)(uint32_t)net->act_counter, 1, st));
    if (!net->greedy) net->act_counter += (unsigned long)T;
    // one workgroup per 64 envs and one workgroup per CU (its LDS): beyond two rounds of workgroups (E > 32 768) the graph of
    // launches takes over.  Measured at the end of round 5, persistent / graph, ms per 20-step rollout: TradeAR1-16 32 768 envs
    // 3.86 / 4.40, 65 536: 7.64 / 7.84; Solow 32 768: 2.01 / 1.93, 65 536: 3.94 / 3.39 (GRL_FLAT_PERSIST_GROUPS moves the limit)
    static const int persist_max_groups = getenv("GRL_FLAT_PERSIST_GROUPS") ? atoi(getenv("GRL_FLAT_PERSIST_GROUPS")) : 512;
    if (net->ro_persistent && (E + 63) / 64 <= persist_max_groups) {
        rc = launch_persistent_rollout(net, T);
        if (rc == GRL_OK) { h->step_in_flight = true; return tw ? window_leave(net, T) : GRL_OK; }
        if (rc != GRL_E_SIZE) return rc;
        net->ro_persistent = 0;      // does not fit the LDS of a CU (very long rollouts): the graph path from here on
    }
    // (the graph holds the buffers' addresses: a true-window graph is only replayed while the slab is the one it was captured on)
    if (net->ro_graph && net->ro_graph_T == T && net->ro_graph_ep == (h->ep_total != nullptr) && net->ro_graph_greedy == net->greedy &&
        net->ro_graph_tw == (tw ? 1 : 0) && (!tw || net->ro_graph_slab == net->ro_slab)) {
        PAAC_HIP(net, hipGraphLaunch(net->ro_graph, st));
    } else {
        if (net->ro_graph) { (void)hipGraphExecDestroy(net->ro_graph); net->ro_graph = nullptr; }
        // ~9 tiny operations per step: capture them once into a graph; every argument is a device pointer or a constant
        const bool capturing = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (!capturing) (void)hipGetLastError();
        rc = enqueue_rollout(net, T);
        if (capturing) {
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamEndCapture(st, &graph);
            if (rc == GRL_OK && e == hipSuccess && graph && hipGraphInstantiate(&net->ro_graph, graph, nullptr, nullptr, 0) == hipSuccess) {
                net->ro_graph_T = T;
                net->ro_graph_ep = h->ep_total != nullptr;
                net->ro_graph_greedy = net->greedy;
                net->ro_graph_tw = tw ? 1 : 0;
                net->ro_graph_slab = net->ro_slab;
            } else {
                net->ro_graph = nullptr;
                (void)hipGetLastError();
            }
            if (graph) (void)hipGraphDestroy(graph);
            if (rc) return rc;
            if (net->ro_graph) PAAC_HIP(net, hipGraphLaunch(net->ro_graph, st));
            else if ((rc = enqueue_rollout(net, T))) return rc;      // capture unavailable: plain launches
        } else if (rc) {
            return rc;
        }
    }
    PAAC_HIP(net, hipGetLastError());
    h->step_in_flight = true;
    return tw ? window_leave(net, T) : GRL_OK;
}

int grl_fnet_set_true_window(grl_fnet *net, int32_t on) {
    if (!net) return GRL_E_INVALID;
    if (net->cfg.static_size != net->cfg.temporal_size)
        return paac_fail(net, GRL_E_INVALID, "grl_fnet_set_true_window: the window's rows are the states, so static_size must equal temporal_size");
    net->true_window = on ? 1 : 0;
    net->ws_resident = 0;      // kept activations are dropped
    net->w_restart_all = 1; net->w_have = 0; net->w_valid = 0;      // every window restarts at the next call
    return GRL_OK;
}

int grl_fnet_read_windows(grl_fnet *net, int32_t first, int32_t count, float *host, size_t bytes) {
    if (!net || (!host && count > 0)) return paac_fail(net, GRL_E_INVALID, "grl_fnet_read_windows: bad argument");
    if (!net->true_window || !net->ro_act || net->T <= 0 || !net->w_valid)
        return paac_fail(net, GRL_E_STATE, "grl_fnet_read_windows: no true-window rollout to read (none yet, or its rows were carried forward)");
    const long TE = (long)net->T * net->h->E;
    const int R = net->cfg.rnn_length, D = net->cfg.temporal_size;
    if (first < 0 || count < 0 || (long)first + count > TE) return paac_fail(net, GRL_E_SIZE, "grl_fnet_read_windows: samples out of range");
    if (bytes != (size_t)count * R * D * 4) return paac_fail(net, GRL_E_SIZE, "grl_fnet_read_windows: wrong size");
    if (count == 0) return GRL_OK;
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    const long total = (long)count * R * D;
    hipLaunchKernelGGL(flat_window_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float *)net->ro_states,
                       (const int32_t *)net->ro_nhist, net->h->E, first, count, R, D, net->d_hist);
    PAAC_HIP(net, hipGetLastError());
    PAAC_HIP(net, hipStreamSynchronize(st));
    PAAC_HIP(net, hipMemcpy(host, net->d_hist, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_fnet_set_greedy(grl_fnet *net, int32_t on) {
    if (!net) return GRL_E_INVALID;
    net->greedy = on ? 1 : 0;
    return GRL_OK;
}

int grl_fnet_eval(grl_fnet *net, int32_t max_steps, int32_t trace_steps, int32_t greedy) {
    if (!net) return GRL_E_INVALID;
    if (max_steps < 1 || trace_steps < 0) return paac_fail(net, GRL_E_INVALID, "grl_fnet_eval: max_steps >= 1, trace_steps >= 0");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = check_env(net);
    if (rc) return rc;
    if (trace_steps > max_steps) trace_steps = max_steps;
    if ((rc = ensure_eval_buffers(net, trace_steps))) return rc;
    if ((rc = launch_eval(net, max_steps, trace_steps, greedy))) return rc;
    if (!greedy) net->act_counter += (unsigned long)max_steps;      // later rollouts never reuse the evaluation's noise
    net->ev_trace = trace_steps;
    net->ev_played = -1;
    net->w_restart_all = 1;      // the handle is reset below: every window restarts
    // the handle's full reset (for Solow with the tape draw), as grl_reset(h, NULL, 0) enqueues it
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E;
    hipStream_t st = h->stream;
    if ((rc = launch_iota(h, h->done_list, E))) return paac_fail(net, rc, h->err);
    net->ev_reset_count = E;
    PAAC_HIP(net, hipMemcpyAsync(h->done_count, &net->ev_reset_count, 4, hipMemcpyHostToDevice, st));
    rc = solow ? solow_launch_reset(h, h->done_list, h->done_count, E, true) : trade_launch_reset(h, h->done_list, h->done_count, E);
    if (rc) return paac_fail(net, rc, h->err);
    return GRL_OK;
}

int grl_fnet_read_eval(grl_fnet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return paac_fail(net, GRL_E_INVALID, "grl_fnet_read_eval: bad argument");
    if (net->ev_played == -2) return paac_fail(net, GRL_E_STATE, "grl_fnet_read_eval: no evaluation yet");
    hipSetDevice(net->h->cfg.device_id);
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t E = net->h->E, S0 = net->cfg.static_size, A = net->cfg.num_actions;
    if (net->ev_played < 0) {      // steps the call played = the longest episode
        std::vector<int32_t> len(E);
        PAAC_HIP(net, hipMemcpy(len.data(), net->ev_len, E * 4, hipMemcpyDeviceToHost));
        int32_t mx = 0;
        for (int32_t l : len) mx = l > mx ? l : mx;
        net->ev_played = mx;
    }
    const size_t SE = (size_t)(net->ev_trace < net->ev_played ? net->ev_trace : net->ev_played) * E;
    struct { const char *name; const void *p; size_t n; } tab[] = {
        {"total_reward", net->ev_total, E * 8}, {"length", net->ev_len, E * 4}, {"finished", net->ev_fin, E},
        {"states", net->ev_states, SE * S0 * 4}, {"nhist", net->ev_nhist, SE * 4}, {"mu", net->ev_mu, SE * A * 4},
        {"sigma", net->ev_sigma, SE * A * 4}, {"raw", net->ev_raw, SE * A * 4}, {"actions", net->ev_act, SE * A * 4},
        {"values", net->ev_val, SE * 4}, {"rewards", net->ev_rew, SE * 4}, {"dones", net->ev_done, SE * 4}};
    for (auto &e : tab)
        if (!strcmp(which, e.name)) {
            if (bytes != e.n) return paac_fail(net, GRL_E_SIZE, std::string("grl_fnet_read_eval: wrong size for ") + which);
            if (bytes) PAAC_HIP(net, hipMemcpy(host, e.p, bytes, hipMemcpyDeviceToHost));
            return GRL_OK;
        }
    return paac_fail(net, GRL_E_INVALID, std::string("grl_fnet_read_eval: unknown buffer ") + which);
}

// Debug / profiling: attach a timestamp buffer to the persistent rollout and read the stage clock of workgroup 0 after the next
// rollout (100 MHz constant clock ticks at every barrier of the kernel).  n_out = number of stamps written to out[0..max).
int grl_fnet_rollout_stage_times(grl_fnet *net, int64_t *out, int32_t max, int32_t *n_out) {
    if (!net || !n_out) return GRL_E_INVALID;
    hipSetDevice(net->h->cfg.device_id);
    if (!net->d_ts) {
        int rc = paac_alloc(net, &net->d_ts, 4096);
        if (rc == GRL_OK) rc = paac_alloc(net, &net->d_ts_n, 4);
        *n_out = 0;
        return rc;
    }
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    int n = 0;
    PAAC_HIP(net, hipMemcpy(&n, net->d_ts_n, sizeof(int), hipMemcpyDeviceToHost));
    if (n > max) n = max;
    if (out && n > 0) PAAC_HIP(net, hipMemcpy(out, net->d_ts, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
    *n_out = n;
    return GRL_OK;
}

int grl_fnet_train_rollout(grl_fnet *net, float lr, float *stats_host) {
    if (!net || !net->ro_states || net->T <= 0) return paac_fail(net, GRL_E_STATE, "grl_fnet_train_rollout: no rollout to train on");
    hipSetDevice(net->h->cfg.device_id);
    const int n = net->T * net->h->E;
    if (net->true_window) {
        if (!net->w_valid) return paac_fail(net, GRL_E_STATE, "grl_fnet_train_rollout: the last rollout's windows were carried forward");
        return train_device(net, n, net->ro_states, nullptr, net->ro_act, net->ro_adv, net->ro_y, lr, 1, stats_host, net->ro_nhist, false, net->h->E);
    }
    return train_device(net, n, net->ro_states, nullptr, net->ro_act, net->ro_adv, net->ro_y, lr, 1, stats_host, net->ro_nhist,
                        net->ws_resident != 0);
}

// the gradient step in two halves for callers that exchange gradients themselves (host all-reduce through gloo when no RCCL
// communicator can be formed): _grads leaves the LOCAL mean gradient in the net, nothing is updated
int grl_fnet_train_rollout_grads(grl_fnet *net, float *stats_host) {
    if (!net || !net->ro_states || net->T <= 0) return paac_fail(net, GRL_E_STATE, "grl_fnet_train_rollout_grads: no rollout to train on");
    hipSetDevice(net->h->cfg.device_id);
    const int n = net->T * net->h->E;
    if (net->true_window && !net->w_valid) return paac_fail(net, GRL_E_STATE, "grl_fnet_train_rollout_grads: the last rollout's windows were carried forward");
    int rc = net->true_window
                 ? train_grads_device(net, n, net->ro_states, nullptr, net->ro_act, net->ro_adv, net->ro_y, net->ro_nhist, false, net->h->E)
                 : train_grads_device(net, n, net->ro_states, nullptr, net->ro_act, net->ro_adv, net->ro_y, net->ro_nhist, net->ws_resident != 0);
    if (rc) return rc;
    return train_apply_device(net, 0.f, 0, 1.0f, stats_host);
}

int grl_fnet_set_grads(grl_fnet *n, const float *host, int64_t cnt) { return paac_copy_flat(n, nullptr, n ? n->grads : nullptr, (float *)host, cnt, true); }

int grl_fnet_apply_grads(grl_fnet *net, float lr, float grad_scale, float *stats_host) {
    if (!net || net->last_n <= 0) return paac_fail(net, GRL_E_STATE, "grl_fnet_apply_grads: no gradient pass has run yet");
    hipSetDevice(net->h->cfg.device_id);
    return train_apply_device(net, lr, 1, grad_scale, stats_host);
}

int grl_fnet_comm_init(grl_fnet *net, const void *unique_id, size_t bytes, int32_t rank, int32_t world_size) {
    return paac_comm_init(net, "grl_fnet_comm_init", unique_id, bytes, rank, world_size);
}

int grl_fnet_comm_info(grl_fnet *net, int32_t *count_out, int32_t *user_rank_out, int64_t *allreduce_calls_out,
                       double *allreduce_ms_total_out, float *allreduce_ms_last_out) {
    return paac_comm_info(net, count_out, user_rank_out, allreduce_calls_out, allreduce_ms_total_out, allreduce_ms_last_out);
}

int grl_fnet_comm_broadcast_params(grl_fnet *net, int32_t root) {
    if (net && net->comm) net->ws_resident = 0;      // the parameters may move (every rank but the root)
    return paac_comm_broadcast_params(net, "grl_fnet_comm_broadcast_params", root);
}

int grl_fnet_comm_destroy(grl_fnet *net) { return paac_comm_destroy(net); }

int grl_fnet_read_rollout(grl_fnet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return GRL_E_INVALID;
    if (!net->ro_states) return paac_fail(net, GRL_E_STATE, "grl_fnet_read_rollout: no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    std::string w(which);
    const size_t TE = (size_t)net->T * net->h->E;
    const void *src = nullptr;
    size_t need = TE * 4;
    if (w == "actions") { src = net->ro_act; need = TE * net->cfg.num_actions * 4; }
    else if (w == "values") src = net->ro_val;
    else if (w == "rewards") src = net->ro_rew;
    else if (w == "masks") src = net->ro_mask;
    else if (w == "y") src = net->ro_y;
    else if (w == "adv") src = net->ro_adv;
    else if (w == "boot") { src = net->ro_boot; need = (size_t)net->h->E * 4; }
    else if (w == "states") { src = net->ro_states; need = TE * net->cfg.static_size * 4; }
    else if (w == "histories" && net->true_window) {      // the true windows, dense: grl_fnet_read_windows over every sample
        need = TE * net->cfg.rnn_length * net->cfg.temporal_size * 4;
        if (need != bytes) return paac_fail(net, GRL_E_SIZE, "grl_fnet_read_rollout: 'histories' needs " + std::to_string(need) + " bytes");
        return grl_fnet_read_windows(net, 0, (int32_t)TE, (float *)host, bytes);
    }
    else if (w == "histories") { src = net->ro_hist; need = TE * net->cfg.rnn_length * 8; }
    else if (w == "nhist") { src = net->ro_nhist; need = TE * 4; }
    else return paac_fail(net, GRL_E_INVALID, "grl_fnet_read_rollout: unknown buffer '" + w + "'");
    if (!src) return paac_fail(net, GRL_E_INVALID, "grl_fnet_read_rollout: '" + w + "' does not exist for this env kind");
    if (need != bytes) return paac_fail(net, GRL_E_SIZE, "grl_fnet_read_rollout: '" + w + "' needs " + std::to_string(need) + " bytes");
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    PAAC_HIP(net, hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // extern "C"
