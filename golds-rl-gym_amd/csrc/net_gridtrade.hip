// The A3C grid trader on gfx950: the reference's DiscretePolicyEstimator with num_outputs = 2 (fed_gym/agents/a3c/estimators.py:
// 18-28,155-238,338-417) on a 2-asset TradeAR1 handle -- the GRU trunk shared by one softmax over K grid points PER ASSET and a value
// head, the device-resident rollout and the A3C update in batched form (include/goldsrl_gridtradenet.h, which says how the agent
// is composed from TradeWorker and GridSolowWorker: the reference has no Trade grid worker).
//
// 91 041 + 258 K parameters.  The fourth client of the A3C nets' shared code: the trunk, the LDS layout, the GEMMs, the window
// rules, the GAE and the update are net_a3c_core.inc's, the host scaffold and the rollout loop net_a3c_host.h's.  The towers restate
// net_discrete.hip's (which restates net_gauss.hip's): sharing them through an include would put that file's kernels' code at stake,
// and its compile-time sizes (D = 2, 64 logit rows) are not this net's (D = 5, 2 x 48).  What is this net's own is the head:
//   logits   ONE probs tower with N = O * K output rows; column o * K + j of probs3 is output o, choice j (the row-major reshape
//            (-1, O, K) of the reference), so output o's logits are the K rows at o * K of the dL/dx rows (L_DX, 96 rows: K <= 48)
//   head     wave o owns output o, one lane per sample: softmax, cumulative-sum draw or arg-max, grid value, and in the backward the
//            loss terms and the logits' dz in place.  The two outputs run at the same time on waves 0 and 1; waves 2 and 3 wait at
//            the barrier.  Nothing is serialised on wave 0, and nothing of one output is read by the other's wave.
//   forward  one launch per pass: trunk, probs tower, both softmaxes, value tower, and when acting both draws (one Philox block per
//            env and step: its first uniform for output 0, its second for output 1) or arg-maxes and the two grid values.  A pass
//            that asks for values only (the bootstrap) skips the probs tower.
//   backward recomputes the forward per 64-sample group; slabs [policy P | value P] per workgroup, reduced in a fixed order (no
//            float atomics on gradients)
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

constexpr int GO = 2;         // outputs = assets
constexpr int GTKMAX = 48;    // most grid points per output
enum : uint32_t { RS_GRIDTRADE_ACTION = 21 };    // next to RS_GRID_ACTION = 20 (net_discrete.hip)
constexpr int A3C_DPAD = 5;   // TradeAR1's processed observation with 2 assets, as in net_gauss.hip
constexpr bool A3C_PAD_LAST = true;
constexpr int GD = 5;         // S0 = D = 5

#include "net_a3c_core.inc"

constexpr int L_LG = L_DX;    // logits -> probs -> their dz: output o at rows o * K
static_assert(GO * GTKMAX <= NX, "the logit rows overflow the dL/dx rows");

// ---- the towers on the trunk's x, restated from net_discrete.hip (see the file comment)
// a policy tower x -> 256 ReLU -> 128 ReLU -> N; the last layer's pre-activations go to the rows at `out`
template <bool LOOP>
__device__ __forceinline__ void gt_tower3_fwd(const float *P, float *lds, long w1, long b1, long w2, long b2, long w3, long b3, int N, float *out) {
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    mm_fwd(P + w1, NW1, P + b1, X, NX, NW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, NW2, P + b2, H1, NW1, NW2, H2, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, N, P + b3, H2, NW2, N, out, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// the value head x -> 256 tanh -> 1: its pre-scale output in row 0 of the O rows
template <bool LOOP, typename ARGS>
__device__ __forceinline__ void gt_value_fwd(const ARGS &a, float *lds) {
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *O = lds + L_O * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    const float *P = a.P;
    mm_fwd(P + a.o.v1w, NW1, P + a.o.v1b, X, NX, NW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, NW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// back through the policy tower whose last layer's dz (N rows) is at dZ = the DX rows; d x into the DX rows: the weight gradient and
// the in-place dx of layer 3 have consumed dZ before the last mm_dx overwrites it
__device__ __forceinline__ void gt_tower3_bwd(const float *P, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, int N,
                                              const float *dZ) {
    float *X = lds + L_X * LS, *DX = lds + L_DX * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS;
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    __syncthreads();
    mm_wgrad(H2, dZ, NW2, N, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w3, NW2, N, dZ, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, NW1, NW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w2, NW1, NW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, NX, NW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, NX, NW1, H1, DX, false, wave, lane);
    __syncthreads();
}

// back through the value head behind gt_value_fwd: row 0 of the O rows holds dz of the output (wave 0 wrote it; the barrier is
// here); weight gradients to Gv, d x into the DX rows
template <typename ARGS>
__device__ __forceinline__ void gt_value_bwd(const ARGS &a, float *lds, float *Gv, int wave, int lane) {
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

struct GOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, p1w, p1b, p2w, p2b, p3w, p3b, v1w, v1b, v2w, v2b, total;
};

static GOff gridtrade_offsets(int K) {
    GOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((GD + NH) * 2 * NH); o.gb = take(2 * NH); o.cw = take((GD + NH) * NH); o.cb = take(NH);
    o.tw = take(NH * 2 * NH); o.tb = take(2 * NH); o.s1w = take(GD * 2 * NH); o.s1b = take(2 * NH); o.s2w = take(2 * NH * NH); o.s2b = take(NH);
    o.p1w = take(NX * NW1); o.p1b = take(NW1); o.p2w = take(NW1 * NW2); o.p2b = take(NW2); o.p3w = take(NW2 * GO * K); o.p3b = take(GO * K);
    o.v1w = take(NX * NW1); o.v1b = take(NW1); o.v2w = take(NW1); o.v2b = take(1);
    o.total = p;
    return o;
}

struct GArgs {
    const float *P;
    GOff o;
    int n, R, K;
    float scale;
    double lb, ub;                      // the grid's ends
    const float *states, *win;          // (n,5) (n,R,5)
    const float *gate;                  // (n) or null: only samples with gate != 0 are evaluated
    // forward outputs (any may be null)
    float *probs, *vals;                // (n,O,K) (n)
    // acting (act != null): one sample per env
    float *act;                         // (n,O) the grid values the env is stepped with
    int32_t *choice_out;                // (n,O)
    int greedy;                         // the arg-maxes, nothing is drawn
    uint64_t seed;
    uint32_t env_off, counter;
    // backward
    const int32_t *choice;              // (n,O)
    const float *adv, *tgt, *wt;        // wt may be null (all 1)
    float mult;
    float *slab;                        // [blocks][2][P]
    float *scratch;                     // [blocks][a3c_scratch_trunk_rows][64]
    double *stats64;                    // policy loss, value loss, weighted entropy sum (over both outputs), weight sum
};

template <bool LOOP>
__device__ __forceinline__ void gt_probs_fwd(const GArgs &a, float *lds) {
    gt_tower3_fwd<LOOP>(a.P, lds, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, GO * a.K, lds + L_LG * LS);
}

// ---- the head of ONE output, one lane per sample: column `lane` of the K rows at PR = the output's first logit row (stride
// LS = 65: conflict-free down a column).  Sequential float32 arithmetic in index order, one operation per statement
// (-ffp-contract=off).  Restated from net_discrete.hip's disc_* for the reason the towers are.
// tf.nn.softmax over the last axis of (n, O, K), in place: max-subtracted, the sum in index order
__device__ __forceinline__ void gt_softmax(float *PR, int K, int lane) {
    float m = PR[lane];
    for (int j = 1; j < K; ++j) m = fmaxf(m, PR[j * LS + lane]);
    float sum = 0.f;
    for (int j = 0; j < K; ++j) {
        const float d = PR[j * LS + lane] - m;
        const float e = expf(d);
        PR[j * LS + lane] = e;
        sum += e;
    }
    for (int j = 0; j < K; ++j) PR[j * LS + lane] = PR[j * LS + lane] / sum;
}

// get_random_discrete_action (worker.py:223-227) per output: the first j with u < the float32 cumulative sum, 0 if none
__device__ __forceinline__ int gt_choose(const float *PR, int K, int lane, double u) {
    float c = 0.f;
    int ch = 0;
    bool found = false;
    for (int j = 0; j < K; ++j) {
        c += PR[j * LS + lane];
        if (!found && u < (double)c) { ch = j; found = true; }
    }
    return ch;
}

// np.argmax per output: the first index of the largest probability
__device__ __forceinline__ int gt_greedy(const float *PR, int K, int lane) {
    float best = PR[lane];
    int ch = 0;
    for (int j = 1; j < K; ++j) {
        const float p = PR[j * LS + lane];
        if (p > best) { best = p; ch = j; }
    }
    return ch;
}

// idx_to_grid (worker.py:349): np.linspace(lb, ub, K)[ch] in float64 -- lb + ch * step with step = (ub - lb) / (K - 1), the last
// point ub itself -- as the float32 the env takes.  Host and device: grl_gtnet_create checks the centre with it.
__host__ __device__ inline float gt_grid(int ch, int K, double lb, double ub) {
    const double step = (ub - lb) / (double)(K - 1);
    return (float)(ch == K - 1 ? ub : lb + (double)ch * step);
}

// what wave o < GO does when the net acts for sample s: output o's choice and grid value
__device__ __forceinline__ int gt_act(const GArgs &a, const float *PRo, int o, int lane, int s) {
    if (a.greedy) return gt_greedy(PRo, a.K, lane);
    double u0, u1;      // one Philox block per (env, step): its first uniform serves output 0, its second output 1
    u01_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GRIDTRADE_ACTION, 0u), u0, u1);
    return gt_choose(PRo, a.K, lane, o == 0 ? u0 : u1);
}

// one launch per forward pass (predict, a rollout step, the bootstrap); with a.act: the draws or the arg-maxes and the grid values
__global__ __launch_bounds__(256) void gt_forward_kernel(GArgs a) {
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *PR = lds + L_LG * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane, K = a.K, OK = GO * K;
    const bool valid = s < a.n;
    bool on = valid;
    if (a.gate) {      // every wave sees the same 64 samples: the exit is uniform over the workgroup
        on = valid && a.gate[s] != 0.f;
        if (__ballot(on) == 0ull) return;
    }
    a3c_trunk<GD, GD, false>(a, lds, sbase, nullptr);
    if (a.probs || a.act) {      // uniform: the bootstrap asks for values only
        gt_probs_fwd<false>(a, lds);
        float *PRo = PR + (wave < GO ? wave : 0) * K * LS;
        if (wave < GO) gt_softmax(PRo, K, lane);
        __syncthreads();
        if (a.probs) {           // (n,O,K): the group's rows are contiguous and row o * K + j is element (o, j): coalesced
            const int cnt = (a.n - sbase < 64 ? a.n - sbase : 64) * OK;
            for (int i = threadIdx.x; i < cnt; i += 256) {
                const int sl = i / OK, j = i - sl * OK;
                a.probs[(size_t)sbase * OK + i] = PR[j * LS + sl];
            }
        }
        if (a.act && valid && wave < GO) {
            const int ch = gt_act(a, PRo, wave, lane, s);
            a.choice_out[(size_t)s * GO + wave] = ch;
            a.act[(size_t)s * GO + wave] = gt_grid(ch, K, a.lb, a.ub);
        }
    }
    if (a.vals) {                // uniform
        gt_value_fwd<false>(a, lds);
        if (on && wave == 0) a.vals[s] = a.scale * O[lane];
    }
}

// Losses (estimators.py:206-212, 377-378), per sample with coefficient c = grad_mult * weight and cp = c * adv:
//   policy  cp * sum_o -log(p_{o,ch_o} + 1e-7);  dz_{o,j} = cp * p_{o,ch_o} / (p_{o,ch_o} + 1e-7) * (p_{o,j} - [j == ch_o])
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
//   entropy the mean over o of -sum_j p_{o,j} log(p_{o,j} + 1e-7) (estimators.py:206), reported only
// Wave o sums output o's terms and writes its dz in place; wave 0 also the value loss.  The workgroup loops over groups blockIdx.x,
// + gridDim.x, ..; its slab holds [policy P | value P] (cleared by the caller).
__global__ __launch_bounds__(256, 1) void gt_backward_kernel(GArgs a) {
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
        const int len = a3c_length(a.win + (size_t)ss * a.R * GD, a.R, GD);
        a3c_trunk<GD, GD, true>(a, lds, sbase, scr);
        // ---- probs tower: each output's dz over its own probabilities, in place, on its own wave
        gt_probs_fwd<true>(a, lds);
        if (wave < GO) {
            float *PRo = PR + wave * K * LS;
            gt_softmax(PRo, K, lane);
            int ch = a.choice[(size_t)ss * GO + wave];
            ch = ch < 0 ? 0 : (ch >= K ? K - 1 : ch);      // the host checks its samples; the rollout's are in range
            const float pc = PRo[ch * LS + lane], f = cp * (pc / (pc + 1e-7f));
            float h = 0.f;
            for (int j = 0; j < K; ++j) {
                const float p = PRo[j * LS + lane];
                h += p * logf(p + 1e-7f);
                PRo[j * LS + lane] = f * (p - (j == ch ? 1.0f : 0.0f));
            }
            if (valid && wt != 0.f) {      // weight-0 samples add nothing
                lp += (double)(cp * -logf(pc + 1e-7f));
                ent += (double)wt * (double)(-h);
                if (wave == 0) wsum += (double)wt;
            }
        }
        gt_tower3_bwd(a.P, lds, Gp, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, GO * K, PR);
        a3c_trunk_bwd<GD, GD, true>(a, lds, sbase, scr, Gp, len);
        // ---- value head
        gt_value_fwd<true>(a, lds);
        if (wave == 0) {
            const float v = a.scale * O[lane], tg = a.tgt[ss], dv = v - tg;
            O[lane] = c * dv;                               // d/dz of c * 0.5 (scale z - t)^2 / scale
            if (valid) lv += (double)(c * 0.5f * dv * dv / a.scale);
        }
        gt_value_bwd(a, lds, Gv, wave, lane);
        a3c_trunk_bwd<GD, GD, true>(a, lds, sbase, scr, Gv, len);
    }
    // wave o < GO summed output o's terms; wave 0 also the value loss and the weights
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lp += __shfl_xor(lp, d); lv += __shfl_xor(lv, d); ent += __shfl_xor(ent, d); wsum += __shfl_xor(wsum, d);
    }
    if (lane == 0 && wave < GO) {
        atomicAdd(&a.stats64[0], lp);
        atomicAdd(&a.stats64[2], ent);
        if (wave == 0) { atomicAdd(&a.stats64[1], lv); atomicAdd(&a.stats64[3], wsum); }
    }
}

#include "net_gridtrade_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"

struct grl_gtnet : grl::A3cNet {
    grl_gtnet_config cfg;
    grl::GOff off;
    int K;                                        // grid points per output; S0 = D = 5, the processed observation
    // the head's host-sample staging, rollout buffers and evaluation trace
    float *d_probs;
    int32_t *d_choice;
    float *ro_probs, *ro_act;                     // ro_act (T,E,O): the grid values each env was stepped with
    int32_t *ro_choice;
    // always_bootstrap is 0 (Trade episodes end terminally): the rollout loop's terminal-pass buffers do not exist
    float *ro_term_st = nullptr, *ro_term_wn = nullptr, *ro_term_val = nullptr, *term_obs = nullptr;
    float *ev_act;                                // (E,O): the evaluation step's actions
    int32_t *ev_choice;
};

namespace grl {

static GArgs gargs(grl_gtnet *net, int n, const float *states, const float *win) {
    GArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.K = net->K; a.scale = net->cfg.scale;
    a.lb = net->cfg.grid_lb; a.ub = net->cfg.grid_ub;
    a.states = states; a.win = win; a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_gtnet *net, const GArgs &a) {
    hipLaunchKernelGGL(gt_forward_kernel, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_gtnet *net, int n, const float *states, const float *win, const int32_t *choice, const float *adv, const float *tgt,
                        const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = a3c_train_begin(net, n, a3c_scratch_trunk_rows(net->cfg.rnn_length), &blocks);
    if (rc) return rc;
    GArgs a = gargs(net, n, states, win);
    a.choice = choice; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    hipLaunchKernelGGL(gt_backward_kernel, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    return a3c_train_finish(net, blocks, net->off.p1w, (double)GO, lr0, apply, stats_host);
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_gtnet_config_default(grl_gtnet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_gtnet_config);
    cfg->rnn_length = 20; cfg->max_samples = 8192; cfg->lr_decay_steps = 100000; cfg->always_bootstrap = 0;
    cfg->num_choices = 17; cfg->num_outputs = GO;
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
            if (cfg->num_outputs != h->cfg.n_assets || h->cfg.n_assets != GO) {
                msg = "num_outputs " + std::to_string(cfg->num_outputs) + " and the handle's " + std::to_string(h->cfg.n_assets) +
                      " assets: the device net has one output per asset and exists for " + std::to_string(GO) + " assets";
                return msg.c_str();
            }
            if (range) return range;
            if (cfg->num_choices < 2 || cfg->num_choices > GTKMAX || !(cfg->grid_lb < cfg->grid_ub)) {
                msg = "num_choices " + std::to_string(cfg->num_choices) + ": 2.." + std::to_string(GTKMAX) + " (" + std::to_string(GO) +
                      " outputs share the " + std::to_string(NX) + " logit rows), grid_lb < grid_ub";
                return msg.c_str();
            }
            if (cfg->always_bootstrap != 0) return "a TradeAR1 handle needs always_bootstrap = 0";
            // a symmetric grid with an odd number of points holds: its centre must be exactly 0.0f (goldsrl_gridtradenet.h)
            const int K = cfg->num_choices;
            if ((K & 1) && cfg->grid_lb == -cfg->grid_ub && gt_grid((K - 1) / 2, K, cfg->grid_lb, cfg->grid_ub) != 0.0f)
                return "the centre of the symmetric grid does not come out as exactly 0: choose another num_choices";
            return nullptr;
        },
        [&](grl_gtnet *n, A3cGrow &Al) {
            n->S0 = n->D = GD; n->K = cfg->num_choices;
            n->off = gridtrade_offsets(n->K);
            const size_t ms = cfg->max_samples, E = h->E, OK = (size_t)GO * n->K;
            n->ro_bufs = {a3c_buf("probs", &n->ro_probs, OK), a3c_buf("choices", &n->ro_choice, GO), a3c_buf("actions", &n->ro_act, GO)};
            n->ev_bufs = {a3c_buf("choices", &n->ev_choice, GO), a3c_buf("actions", &n->ev_actions, GO)};
            Al(&n->d_choice, ms * GO); Al(&n->d_probs, ms * OK); Al(&n->ev_act, E * GO);
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
    int rc = a3c_samples_check(net, "grl_gtnet_predict", n, states && windows);
    if (rc || (rc = a3c_stage(net, n, states, windows))) return rc;
    GArgs a = gargs(net, n, net->d_states, net->d_win);
    a.probs = net->d_probs; a.vals = net->d_vals;
    if ((rc = launch_fwd(net, a))) return rc;
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if ((rc = a3c_get(net, probs, net->d_probs, (size_t)n * GO * net->K))) return rc;
    return a3c_get(net, values, net->d_vals, n);
}

int grl_gtnet_train(grl_gtnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *adv,
                    const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    int rc = a3c_samples_check(net, "grl_gtnet_train", n, states && windows && choices && adv && targets);
    if (rc) return rc;
    for (int64_t i = 0; i < (int64_t)n * GO; ++i)
        if (choices[i] < 0 || choices[i] >= net->K) return a3c_fail(net, GRL_E_INVALID, "grl_gtnet_train: a choice outside [0, num_choices)");
    if ((rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_choice, choices, (size_t)n * GO)) ||
        (rc = a3c_stage_targets(net, n, adv, targets, weights)))
        return rc;
    return train_device(net, n, net->d_states, net->d_win, net->d_choice, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult, lr0,
                        apply_update, stats_host);
}

int grl_gtnet_rollout(grl_gtnet *net, int32_t T) {
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, "grl_gtnet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = a3c_ensure_rollout(net, T);
    if (rc) return rc;
    const size_t OK = (size_t)GO * net->K;
    return a3c_rollout_run(
        net, T, h->tr.obs, [&](int n, const float *states, const float *win) { return gargs(net, n, states, win); },
        [&](GArgs &a, size_t o, int t) {
            a.probs = net->ro_probs + o * OK; a.act = net->ro_act + o * GO; a.choice_out = net->ro_choice + o * GO;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
        },
        [&](const GArgs &a) { return launch_fwd(net, a); }, [&](size_t o) { return trade_launch_step(h, net->ro_act + o * GO); });
}

int grl_gtnet_eval(grl_gtnet *net, int32_t max_steps, int32_t trace_steps) {
    int rc = a3c_eval_begin(net, "grl_gtnet_eval", max_steps, &trace_steps);
    if (rc) return rc;
    grl_handle *h = net->h;
    const int E = h->E;
    GEvalArgs v{};
    v.a = gargs(net, E, h->tr.obs, net->win);
    a3c_eval_args(net, v, max_steps, trace_steps);
    v.act = net->ev_act; v.tr_choice = net->ev_choice; v.tr_act = net->ev_actions;
    hipLaunchKernelGGL(gt_eval_kernel, dim3((E + 63) / 64), dim3(256), A3C_LDS, h->stream, v, trade_params(h));
    return a3c_eval_finish(net, trace_steps, [&] { return trade_launch_reset(h, h->done_list, h->done_count, E); });
}

int grl_gtnet_read_eval(grl_gtnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_gtnet_read_eval", which, host, bytes); }

int grl_gtnet_train_rollout(grl_gtnet *net, float lr0, float *stats_host) {
    return a3c_train_rollout(net, "grl_gtnet_train_rollout", [&](int n, float mult) {
        return train_device(net, n, net->ro_states, net->ro_win, net->ro_choice, net->ro_adv, net->ro_tgt, net->ro_wt, mult, lr0, 1, stats_host);
    });
}

int grl_gtnet_read_rollout(grl_gtnet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_gtnet_read_rollout", "", which, host, bytes);
}

}  // extern "C"
