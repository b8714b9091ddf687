// The A3C discrete savings-grid agent on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-28,155-238,338-417 and
// GridSolowWorker, fed_gym/agents/a3c/worker.py:69-341,343-391): the GRU trunk shared by a softmax policy over K savings rates and
// a value head, the device-resident rollout on a Solow handle and the A3C update in batched form (include/goldsrl_discretenet.h).
//
// 90 561 + 129 K parameters.  The third client of the A3C nets' shared code: the trunk, the LDS layout, the GEMMs, the window rules,
// the GAE and the update are net_a3c_core.inc's, the host scaffold and the rollout loop net_a3c_host.h's.  What is this net's own:
// the towers in a form with the head's rows as a parameter, the softmax head, the sampler, the arg-max and the loss behind them.
//   forward   one launch per pass: trunk, probs tower, softmax, value tower, and when acting the draw or the arg-max and the grid
//             value.  A pass that asks for values only (the bootstraps) skips the probs tower.
//   backward  recomputes the forward per 64-sample group; with a single policy tower nothing is parked in scratch.  Slabs
//             [policy P | value P] per workgroup, reduced in a fixed order (no float atomics on gradients)
//   eval      whole greedy episodes in one launch (net_discrete_eval.inc): a workgroup keeps its 64 envs, probs tower only
// The K logits (up to 64 rows) do not fit the 16 head rows of the shared layout, and the layout does not grow: they live in the
// dL/dx rows (L_DX, 96 rows), free in the forward, and in the backward free until the tower's last mm_dx writes them -- by then the
// weight gradient and the in-place dx of layer 3 have consumed the logits' dz.  The value head stays in the O rows.
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

constexpr int DKMAX = 64;     // most grid points
enum : uint32_t { RS_GRID_ACTION = 20 };    // next to RS_GATED_ACTION = 18 (net_gated.hip) and RS_GAUSS_ACTION = 19 (net_gauss.hip)
constexpr int A3C_DPAD = 2;   // Solow's processed observation
constexpr bool A3C_PAD_LAST = true;
constexpr int DD = 2;         // S0 = D = 2

#include "net_a3c_core.inc"

// The towers on the trunk's x.  They restate net_gauss.hip's gauss_tower_fwd / gauss_tower_bwd and its value head with the second
// layer's activation and the head's rows as parameters; the Gaussian net keeps its own, because routing it through these changed
// its kernels' code.
// A policy tower x -> 256 ReLU -> 128 ACT2 -> N; the last layer's pre-activations go to the rows at `out`
template <bool LOOP, int ACT2>
__device__ __forceinline__ void a3c_tower3_fwd(const float *P, float *lds, long w1, long b1, long w2, long b2, long w3, long b3, int N, float *out) {
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    mm_fwd(P + w1, NW1, P + b1, X, NX, NW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, NW2, P + b2, H1, NW1, NW2, H2, ACT2, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, N, P + b3, H2, NW2, N, out, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// the value head x -> 256 tanh -> 1: its pre-scale output in row 0 of the O rows
template <bool LOOP, typename ARGS>
__device__ __forceinline__ void a3c_value_fwd(const ARGS &a, float *lds) {
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *O = lds + L_O * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    const float *P = a.P;
    mm_fwd(P + a.o.v1w, NW1, P + a.o.v1b, X, NX, NW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, NW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// back through a policy tower whose last layer's dz (N rows) is at dZ; d x (=|+=) into the DX rows.  dZ may be the DX rows
// themselves where accumulate is false: the weight gradient and the in-place dx of layer 3 have consumed it before the last mm_dx
// writes them.
template <int ACT2>
__device__ __forceinline__ void a3c_tower3_bwd(const float *P, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, int N,
                                               const float *dZ, bool accumulate) {
    float *X = lds + L_X * LS, *DX = lds + L_DX * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS;
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    __syncthreads();
    mm_wgrad(H2, dZ, NW2, N, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<ACT2>(P + w3, NW2, N, dZ, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, NW1, NW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w2, NW1, NW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, NX, NW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, NX, NW1, H1, DX, accumulate, wave, lane);
    __syncthreads();
}

// back through the value head behind a3c_value_fwd: row 0 of the O rows holds dz of the output (wave 0 wrote it; the barrier is
// here); weight gradients to Gv, d x into the DX rows
template <typename ARGS>
__device__ __forceinline__ void a3c_value_bwd(const ARGS &a, float *lds, float *Gv, int wave, int lane) {
    float *O = lds + L_O * LS, *H1 = lds + L_H1 * LS;
    __syncthreads();
    mm_wgrad(H1, O, NW1, 1, Gv + a.o.v2w, Gv + a.o.v2b, wave, lane);
    __syncthreads();
    for (int i = wave; i < NW1; i += 4) {
        const float h = H1[i * LS + lane];
        H1[i * LS + lane] = a.P[a.o.v2w + i] * O[lane] * (1.0f - h * h);
    }
    __syncthreads();
    mm_wgrad(lds + L_X * LS, H1, NX, NW1, Gv + a.o.v1w, Gv + a.o.v1b, wave, lane);
    mm_dx(a.P + a.o.v1w, NX, NW1, H1, lds + L_DX * LS, false, wave, lane);
}

constexpr int L_LG = L_DX;    // logits -> probs -> their dz
static_assert(DKMAX <= NX, "the logit rows overflow the dL/dx rows");

struct DOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, p1w, p1b, p2w, p2b, p3w, p3b, v1w, v1b, v2w, v2b, total;
};

static DOff discrete_offsets(int K) {
    DOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((DD + NH) * 2 * NH); o.gb = take(2 * NH); o.cw = take((DD + NH) * NH); o.cb = take(NH);
    o.tw = take(NH * 2 * NH); o.tb = take(2 * NH); o.s1w = take(DD * 2 * NH); o.s1b = take(2 * NH); o.s2w = take(2 * NH * NH); o.s2b = take(NH);
    o.p1w = take(NX * NW1); o.p1b = take(NW1); o.p2w = take(NW1 * NW2); o.p2b = take(NW2); o.p3w = take(NW2 * K); o.p3b = take(K);
    o.v1w = take(NX * NW1); o.v1b = take(NW1); o.v2w = take(NW1); o.v2b = take(1);
    o.total = p;
    return o;
}

struct DArgs {
    const float *P;
    DOff o;
    int n, R, K;
    float scale;
    double lb, ub;                      // the grid's ends
    const float *states, *win;          // (n,2) (n,R,2)
    const float *gate;                  // (n) or null: only samples with gate != 0 are evaluated (the terminal value pass)
    // forward outputs (any may be null)
    float *probs, *vals;                // (n,K) (n)
    // acting (act != null): one sample per env
    float *act;                         // (n) the grid value the env is stepped with
    int32_t *choice_out;                // (n)
    int greedy;                         // the arg-max, nothing is drawn
    uint64_t seed;
    uint32_t env_off, counter;
    // backward
    const int32_t *choice;
    const float *adv, *tgt, *wt;        // wt may be null (all 1)
    float mult;
    float *slab;                        // [blocks][2][P]
    float *scratch;                     // [blocks][a3c_scratch_trunk_rows][64]
    double *stats64;                    // policy loss, value loss, weighted entropy sum, weight sum
};

template <bool LOOP>
__device__ __forceinline__ void disc_probs_fwd(const DArgs &a, float *lds) {
    a3c_tower3_fwd<LOOP, FACT_RELU>(a.P, lds, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, a.K, lds + L_LG * LS);
}

// The head, one lane per sample: column `lane` of the K rows at PR (stride LS = 65: conflict-free down a column).  Sequential
// float32 arithmetic in index order (-ffp-contract=off).
// tf.nn.softmax in place: max-subtracted, the sum in index order
__device__ __forceinline__ void disc_softmax(float *PR, int K, int lane) {
    float m = PR[lane];
    for (int j = 1; j < K; ++j) m = fmaxf(m, PR[j * LS + lane]);
    float sum = 0.f;
    for (int j = 0; j < K; ++j) {
        const float e = expf(PR[j * LS + lane] - m);
        PR[j * LS + lane] = e;
        sum += e;
    }
    for (int j = 0; j < K; ++j) PR[j * LS + lane] = PR[j * LS + lane] / sum;
}

// get_random_discrete_action (worker.py:223-227): (u < cum_probs).argmax() -- the first i with u < the float32 cumulative sum, 0 if none
__device__ __forceinline__ int disc_choose(const float *PR, int K, int lane, double u) {
    float c = 0.f;
    int ch = 0;
    bool found = false;
    for (int j = 0; j < K; ++j) {
        c += PR[j * LS + lane];
        if (!found && u < (double)c) { ch = j; found = true; }
    }
    return ch;
}

// np.argmax: the first index of the largest probability
__device__ __forceinline__ int disc_greedy(const float *PR, int K, int lane) {
    float best = PR[lane];
    int ch = 0;
    for (int j = 1; j < K; ++j) {
        const float p = PR[j * LS + lane];
        if (p > best) { best = p; ch = j; }
    }
    return ch;
}

// idx_to_grid (worker.py:349): np.linspace(lb, ub, K)[ch] in float64 -- lb + ch * step with step = (ub - lb) / (K - 1), the last
// point ub itself -- as the float32 the env takes
__device__ __forceinline__ float disc_grid(int ch, int K, double lb, double ub) {
    const double step = (ub - lb) / (double)(K - 1);
    return (float)(ch == K - 1 ? ub : lb + (double)ch * step);
}

// one launch per forward pass (predict, a rollout step, the bootstraps); with a.act: the draw or the arg-max and the grid value
__global__ __launch_bounds__(256) void disc_forward_kernel(DArgs a) {
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *PR = lds + L_LG * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane, K = a.K;
    const bool valid = s < a.n;
    bool on = valid;
    if (a.gate) {      // every wave sees the same 64 samples: the exit is uniform over the workgroup
        on = valid && a.gate[s] != 0.f;
        if (__ballot(on) == 0ull) return;
    }
    a3c_trunk<DD, DD, false>(a, lds, sbase, nullptr);
    if (a.probs || a.act) {      // uniform: the bootstraps ask for values only
        disc_probs_fwd<false>(a, lds);
        if (wave == 0) disc_softmax(PR, K, lane);
        __syncthreads();
        if (a.probs) {           // (n,K) rows of the group are contiguous: coalesced
            const int cnt = (a.n - sbase < 64 ? a.n - sbase : 64) * K;
            for (int i = threadIdx.x; i < cnt; i += 256) {
                const int sl = i / K, j = i - sl * K;
                a.probs[(size_t)sbase * K + i] = PR[j * LS + sl];
            }
        }
        if (a.act && valid && wave == 0) {
            int ch;
            if (a.greedy) {
                ch = disc_greedy(PR, K, lane);
            } else {
                double u, u1;
                u01_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GRID_ACTION, 0u), u, u1);
                ch = disc_choose(PR, K, lane, u);
            }
            a.choice_out[s] = ch;
            a.act[s] = disc_grid(ch, K, a.lb, a.ub);
        }
    }
    if (a.vals) {                // uniform
        a3c_value_fwd<false>(a, lds);
        if (on && wave == 0) a.vals[s] = a.scale * O[lane];
    }
}

// Losses (estimators.py:206-212, 377-378), per sample with coefficient c = grad_mult * weight:
//   policy  c * adv * -log(p_choice + 1e-7);  dz_j = c * adv * p_choice / (p_choice + 1e-7) * (p_j - [j == choice])
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
//   entropy -sum_j p_j log(p_j + 1e-7), reported only
// The workgroup loops over groups blockIdx.x, + gridDim.x, ..; its slab holds [policy P | value P] (cleared by the caller).
__global__ __launch_bounds__(256, 1) void disc_backward_kernel(DArgs a) {
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *PR = lds + L_LG * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = a.K;
    const long Pn = a.o.total;
    float *Gp = a.slab + (size_t)blockIdx.x * 2 * Pn, *Gv = Gp + Pn;
    float *scr = a.scratch + (size_t)blockIdx.x * a3c_scratch_trunk_rows(a.R) * 64;
    const int groups = (a.n + 63) / 64;
    double lp = 0.0, lv = 0.0, ent = 0.0, wsum = 0.0;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int sbase = grp * 64, s = sbase + lane;
        const bool valid = s < a.n;
        const int ss = valid ? s : 0;
        const float wt = valid ? (a.wt ? a.wt[ss] : 1.0f) : 0.f;
        const float c = a.mult * wt, adv = a.adv[ss], cp = c * adv;
        const int len = a3c_length(a.win + (size_t)ss * a.R * DD, a.R, DD);
        a3c_trunk<DD, DD, true>(a, lds, sbase, scr);
        // ---- probs tower: the logits' dz over the probabilities, in place
        disc_probs_fwd<true>(a, lds);
        if (wave == 0) {
            disc_softmax(PR, K, lane);
            int ch = a.choice[ss];
            ch = ch < 0 ? 0 : (ch >= K ? K - 1 : ch);      // the host checks its samples; the rollout's are in range
            const float pc = PR[ch * LS + lane], f = cp * (pc / (pc + 1e-7f));
            float h = 0.f;
            for (int j = 0; j < K; ++j) {
                const float p = PR[j * LS + lane];
                h += p * logf(p + 1e-7f);
                PR[j * LS + lane] = f * (p - (j == ch ? 1.0f : 0.0f));
            }
            if (valid && wt != 0.f) {      // weight-0 samples add nothing
                lp += (double)(cp * -logf(pc + 1e-7f));
                ent += (double)wt * (double)(-h);
                wsum += (double)wt;
            }
        }
        a3c_tower3_bwd<FACT_RELU>(a.P, lds, Gp, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, K, PR, false);
        a3c_trunk_bwd<DD, DD, true>(a, lds, sbase, scr, Gp, len);
        // ---- value head
        a3c_value_fwd<true>(a, lds);
        if (wave == 0) {
            const float v = a.scale * O[lane], tg = a.tgt[ss], dv = v - tg;
            O[lane] = c * dv;                               // d/dz of c * 0.5 (scale z - t)^2 / scale
            if (valid) lv += (double)(c * 0.5f * dv * dv / a.scale);
        }
        a3c_value_bwd(a, lds, Gv, wave, lane);
        a3c_trunk_bwd<DD, DD, true>(a, lds, sbase, scr, Gv, len);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lp += __shfl_xor(lp, d); lv += __shfl_xor(lv, d); ent += __shfl_xor(ent, d); wsum += __shfl_xor(wsum, d);
    }
    if (lane == 0 && wave == 0) {
        atomicAdd(&a.stats64[0], lp);
        atomicAdd(&a.stats64[1], lv);
        atomicAdd(&a.stats64[2], ent);
        atomicAdd(&a.stats64[3], wsum);
    }
}

#include "net_discrete_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"

struct grl_dnet : grl::A3cNet {
    grl_dnet_config cfg;
    grl::DOff off;
    int K;                                        // grid points; S0 = D = 2, the processed observation
    // the head's host-sample staging, rollout buffers and evaluation trace
    float *d_probs;
    int32_t *d_choice;
    float *ro_probs, *ro_act;                     // ro_act (T,E): the grid value each env was stepped with
    int32_t *ro_choice;
    float *ro_term_st, *ro_term_wn, *ro_term_val;
    float *term_obs;
    float *ev_act;                                // (E): the evaluation step's actions
    int32_t *ev_choice;
};

namespace grl {

static DArgs dargs(grl_dnet *net, int n, const float *states, const float *win) {
    DArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.K = net->K; a.scale = net->cfg.scale;
    a.lb = net->cfg.grid_lb; a.ub = net->cfg.grid_ub;
    a.states = states; a.win = win; a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_dnet *net, const DArgs &a) {
    hipLaunchKernelGGL(disc_forward_kernel, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_dnet *net, int n, const float *states, const float *win, const int32_t *choice, const float *adv, const float *tgt,
                        const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = a3c_train_begin(net, n, a3c_scratch_trunk_rows(net->cfg.rnn_length), &blocks);
    if (rc) return rc;
    DArgs a = dargs(net, n, states, win);
    a.choice = choice; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    hipLaunchKernelGGL(disc_backward_kernel, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    return a3c_train_finish(net, blocks, net->off.p1w, 1.0, lr0, apply, stats_host);
}

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
            if (cfg->num_choices < 2 || cfg->num_choices > DKMAX || !(cfg->grid_lb < cfg->grid_ub)) return "num_choices 2..64, grid_lb < grid_ub";
            return cfg->always_bootstrap != 1 ? "a Solow handle needs always_bootstrap = 1" : nullptr;
        },
        [&](grl_dnet *n, A3cGrow &Al) {
            n->S0 = n->D = DD; n->K = cfg->num_choices;
            n->off = discrete_offsets(n->K);
            const size_t ms = cfg->max_samples, E = h->E, K = n->K, W = (size_t)cfg->rnn_length * DD;
            n->ro_bufs = {a3c_buf("probs", &n->ro_probs, K), a3c_buf("choices", &n->ro_choice, 1), a3c_buf("actions", &n->ro_act, 1),
                          a3c_buf("term_values", &n->ro_term_val, 1), a3c_buf("term_states", &n->ro_term_st, DD),
                          a3c_buf("term_windows", &n->ro_term_wn, W)};
            n->ev_bufs = {a3c_buf("choices", &n->ev_choice, 1), a3c_buf("actions", &n->ev_actions, 1)};
            Al(&n->d_choice, ms); Al(&n->d_probs, ms * K); Al(&n->term_obs, E * DD); Al(&n->ev_act, E);
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
    int rc = a3c_samples_check(net, "grl_dnet_predict", n, states && windows);
    if (rc || (rc = a3c_stage(net, n, states, windows))) return rc;
    DArgs a = dargs(net, n, net->d_states, net->d_win);
    a.probs = net->d_probs; a.vals = net->d_vals;
    if ((rc = launch_fwd(net, a))) return rc;
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if ((rc = a3c_get(net, probs, net->d_probs, (size_t)n * net->K))) return rc;
    return a3c_get(net, values, net->d_vals, n);
}

int grl_dnet_train(grl_dnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    int rc = a3c_samples_check(net, "grl_dnet_train", n, states && windows && choices && adv && targets);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (choices[i] < 0 || choices[i] >= net->K) return a3c_fail(net, GRL_E_INVALID, "grl_dnet_train: a choice outside [0, num_choices)");
    if ((rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_choice, choices, n)) ||
        (rc = a3c_stage_targets(net, n, adv, targets, weights)))
        return rc;
    return train_device(net, n, net->d_states, net->d_win, net->d_choice, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult, lr0,
                        apply_update, stats_host);
}

int grl_dnet_rollout(grl_dnet *net, int32_t T) {
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, "grl_dnet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = a3c_ensure_rollout(net, T);
    if (rc) return rc;
    const size_t K = net->K;
    return a3c_rollout_run(
        net, T, h->so.obs, [&](int n, const float *states, const float *win) { return dargs(net, n, states, win); },
        [&](DArgs &a, size_t o, int t) {
            a.probs = net->ro_probs + o * K; a.act = net->ro_act + o; a.choice_out = net->ro_choice + o;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
        },
        [&](const DArgs &a) { return launch_fwd(net, a); }, [&](size_t o) { return solow_launch_step(h, net->ro_act + o, net->term_obs); });
}

int grl_dnet_eval(grl_dnet *net, int32_t max_steps, int32_t trace_steps) {
    int rc = a3c_eval_begin(net, "grl_dnet_eval", max_steps, &trace_steps);
    if (rc) return rc;
    grl_handle *h = net->h;
    const int E = h->E;
    DEvalArgs v{};
    v.a = dargs(net, E, h->so.obs, net->win);
    a3c_eval_args(net, v, max_steps, trace_steps);
    v.act = net->ev_act; v.tr_choice = net->ev_choice; v.tr_act = net->ev_actions;
    hipLaunchKernelGGL(disc_eval_kernel, dim3((E + 63) / 64), dim3(256), A3C_LDS, h->stream, v, solow_params(h));
    return a3c_eval_finish(net, trace_steps, [&] { return solow_launch_reset(h, h->done_list, h->done_count, E, true); });      // with the tape draw
}

int grl_dnet_read_eval(grl_dnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_dnet_read_eval", which, host, bytes); }

int grl_dnet_train_rollout(grl_dnet *net, float lr0, float *stats_host) {
    return a3c_train_rollout(net, "grl_dnet_train_rollout", [&](int n, float mult) {
        return train_device(net, n, net->ro_states, net->ro_win, net->ro_choice, net->ro_adv, net->ro_tgt, net->ro_wt, mult, lr0, 1, stats_host);
    });
}

int grl_dnet_read_rollout(grl_dnet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_dnet_read_rollout", "", which, host, bytes);
}

}  // extern "C"
