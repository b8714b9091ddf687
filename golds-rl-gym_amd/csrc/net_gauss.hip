// The A3C Gaussian agent on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-28,241-417 and the worker loop of
// fed_gym/agents/a3c/worker.py:69-341,394-442): a GRU trunk shared by a Gaussian policy (mu and sigma towers) and a value head,
// the device-resident rollout on a Solow or TradeAR1 handle and the A3C update in batched form (include/goldsrl_gaussnet.h).
//
// 148 547 (Solow) / 149 285 (TradeAR1, 2 assets) parameters.  The trunk, the LDS layout, the window rules and the update are the
// ones the gated trader (net_gated.hip) uses as well (net_a3c_core.inc; on the host net_a3c_host.h): a workgroup of 4 waves owns 64
// samples, activations live in LDS as [feature][sample] rows of LS = 65 floats, every dense layer is an exact-fp32
// v_mfma_f32_32x32x2_f32 GEMM (net_mfma_gemm.inc), the towers run one after another through the same two buffers (256 + 128 rows).
// The kernels are compiled for the two size sets (D = S0 = 2, A = 1 and D = S0 = 5, A = 2).
//   forward   one launch per rollout step: window GRU, trunk, towers, 5 tanh / sigmoid + 1e-3, the draw and the env action
//   backward  recomputes the forward per group (the GRU's per-step activations go to a per-workgroup scratch in global memory).
//             Both heads' gradients need both heads' outputs (nll = log sigma + (a - mu)^2 / 2 sigma^2), and the towers share their
//             LDS rows: the mu tower's two hidden layers are parked in the workgroup's scratch while the sigma tower runs forward and
//             backward, and come back for the mu tower's backward -- 96 KB out and in through L2 instead of a second mu forward.
//             Weight gradients of the groups a workgroup loops over are summed into its private slab [policy P | value P]; the slabs
//             are reduced in a fixed order (bitwise reproducible runs, no float atomics on gradients)
//   update    two float64 sums of squares, clip factors, both RMSProp steps -- on the device
//   eval      whole greedy episodes in one launch (net_gauss_eval.inc): a workgroup keeps its 64 envs, mu tower only
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/goldsrl_gaussnet.h"
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "flat_env_dev.h"

namespace grl {

constexpr int ADMAX = 5;      // largest processed observation (TradeAR1 with 2 assets); Solow: 2
constexpr int AMAXA = 2;      // actions
enum : uint32_t { RS_GAUSS_ACTION = 19 };   // next to RS_GATED_ACTION = 18 (net_gated.hip)
constexpr int A3C_DPAD = ADMAX;
constexpr bool A3C_PAD_LAST = true;

#include "net_a3c_core.inc"

struct AOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, m1w, m1b, m2w, m2b, m3w, m3b, g1w, g1b, g2w, g2b, g3w, g3b, v1w, v1b, v2w, v2b, total;
};

static AOff gauss_offsets(int D, int A) {
    AOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((D + NH) * 2 * NH); o.gb = take(2 * NH); o.cw = take((D + NH) * NH); o.cb = take(NH);
    o.tw = take(NH * 2 * NH); o.tb = take(2 * NH); o.s1w = take(D * 2 * NH); o.s1b = take(2 * NH); o.s2w = take(2 * NH * NH); o.s2b = take(NH);
    o.m1w = take(NX * NW1); o.m1b = take(NW1); o.m2w = take(NW1 * NW2); o.m2b = take(NW2); o.m3w = take(NW2 * A); o.m3b = take(A);
    o.g1w = take(NX * NW1); o.g1b = take(NW1); o.g2w = take(NW1 * NW2); o.g2b = take(NW2); o.g3w = take(NW2 * A); o.g3b = take(A);
    o.v1w = take(NX * NW1); o.v1b = take(NW1); o.v2w = take(NW1); o.v2b = take(1);
    o.total = p;
    return o;
}

struct AArgs {
    const float *P;
    AOff o;
    int n, R;                           // the widths D = S0 (the temporal row is the whole processed state) and A are the kernels' template parameter
    float scale;
    const float *states, *win;          // (n,D) (n,R,D)
    const float *gate;                  // (n) or null: only samples with gate != 0 are evaluated (the terminal value pass)
    // forward outputs (any may be null)
    float *mu, *sigma, *vals;           // (n,A) (n,A) (n)
    // acting (act != null): one sample per env
    float *act;                         // (n,A) the env's action
    float *raw_out;                     // (n,A)
    int tanh_action;                    // TradeAR1: tanh(raw); Solow: the stable sigmoid
    int greedy;                         // raw = mu, nothing is drawn (run_n_steps(stochastic=False), worker.py:180-230)
    uint64_t seed;
    uint32_t env_off, counter;
    // backward
    const float *raw, *adv, *tgt, *wt;  // wt may be null (all 1)
    float mult;
    float *slab;                        // [blocks][2][P]
    float *scratch;                     // [blocks][gauss_scratch_rows][64]
    double *stats64;                    // policy loss, value loss, weighted entropy sum, weight sum
};

// per-workgroup scratch of the recomputed forward: the trunk's rows, then the parked mu tower (256 + 128)
__host__ __device__ inline int gauss_scratch_rows(int R) { return a3c_scratch_trunk_rows(R) + NW1 + NW2; }

// tower 0 = mu, 1 = sigma: x -> 256 ReLU -> 128 tanh -> A (pre-activation, O rows); tower 2 = value: x -> 256 tanh -> 1
template <int D, bool LOOP>
__device__ __forceinline__ void gauss_tower_fwd(const AArgs &a, float *lds, int tower) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS, *O = lds + L_O * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    const float *P = a.P;
    if (tower == 2) {
        mm_fwd(P + a.o.v1w, NW1, P + a.o.v1b, X, NX, NW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, NW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
        __syncthreads();
        return;
    }
    const long w1 = tower ? a.o.g1w : a.o.m1w, b1 = tower ? a.o.g1b : a.o.m1b, w2 = tower ? a.o.g2w : a.o.m2w,
               b2 = tower ? a.o.g2b : a.o.m2b, w3 = tower ? a.o.g3w : a.o.m3w, b3 = tower ? a.o.g3b : a.o.m3b;
    mm_fwd(P + w1, NW1, P + b1, X, NX, NW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, NW2, P + b2, H1, NW1, NW2, H2, FACT_TANH, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, A, P + b3, H2, NW2, A, O, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

__device__ __forceinline__ float gauss_mu(float z) { return 5.0f * tanhf(z); }                   // lb = -5, ub = 5 (estimators.py:283)
__device__ __forceinline__ float gauss_sigma(float z) { return sigmoidf_(z) + 1e-3f; }          // estimators.py:288-290

// what the env is stepped with: SolowWorker.transform_raw_action (worker.py:414-415) as a stable float32 sigmoid, TradeWorker
// (:436-442) tanh per action
__device__ __forceinline__ float gauss_env_action(float raw, int tanh_action) {
    if (tanh_action) return tanhf(raw);
    const float z = expf(-fabsf(raw));
    return raw >= 0.f ? 1.0f / (1.0f + z) : z / (1.0f + z);
}

// one launch per forward pass (predict, a rollout step, the bootstraps); with a.act: the draw and the env action as well
template <int D>
__global__ __launch_bounds__(256) void gauss_forward_kernel(AArgs a) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *MU = lds + L_HEAD * LS, *SG = MU + AMAXA * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane;
    const bool valid = s < a.n;
    bool on = valid;
    if (a.gate) {      // every wave sees the same 64 samples: the exit is uniform over the workgroup
        on = valid && a.gate[s] != 0.f;
        if (__ballot(on) == 0ull) return;
    }
    a3c_trunk<D, D, false>(a, lds, sbase, nullptr);
    gauss_tower_fwd<D, false>(a, lds, 0);
    if (wave < A) MU[wave * LS + lane] = gauss_mu(O[wave * LS + lane]);
    __syncthreads();
    gauss_tower_fwd<D, false>(a, lds, 1);
    if (wave < A) SG[wave * LS + lane] = gauss_sigma(O[wave * LS + lane]);
    __syncthreads();
    gauss_tower_fwd<D, false>(a, lds, 2);
    if (on) {
        if (wave < A) {
            if (a.mu) a.mu[(size_t)s * A + wave] = MU[wave * LS + lane];
            if (a.sigma) a.sigma[(size_t)s * A + wave] = SG[wave * LS + lane];
        }
        if (wave == 0 && a.vals) a.vals[s] = a.scale * O[lane];
    }
    if (a.act && valid && wave < A) {
        // SolowWorker.get_random_action (worker.py:410-412), TradeWorker (:436-442) per action; greedy: a zero in place of the normal
        double nz = 0.0, nz1;
        if (!a.greedy) normal_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GAUSS_ACTION, (uint32_t)wave), nz, nz1);
        const float m = MU[wave * LS + lane];
        const float raw = a.greedy ? m : (float)((double)m + (double)SG[wave * LS + lane] * nz);
        a.raw_out[(size_t)s * A + wave] = raw;
        a.act[(size_t)s * A + wave] = gauss_env_action(raw, a.tanh_action);
    }
}

// back through a 96 -> 256 ReLU -> 128 tanh -> A tower whose dz of the last layer is in the O rows; d x (=|+=) into DX
template <int D>
__device__ __forceinline__ void gauss_tower_bwd(const AArgs &a, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, bool accumulate) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    float *X = lds + L_X * LS, *DX = lds + L_DX * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS, *O = lds + L_O * LS;
    const int tid = a3c_tid(), lane = tid & 63, wave = a3c_wave(tid);
    const float *P = a.P;
    __syncthreads();
    mm_wgrad(H2, O, NW2, A, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_TANH>(P + w3, NW2, A, O, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, NW1, NW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w2, NW1, NW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, NX, NW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, NX, NW1, H1, DX, accumulate, wave, lane);
    __syncthreads();
}

// Losses (estimators.py:292-304, 377-378), per sample with coefficient c = grad_mult * weight:
//   policy  c * adv * sum_actions (0.5 log 2 pi + log sigma + (raw - mu)^2 / (2 sigma^2))
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
// The workgroup loops over groups blockIdx.x, + gridDim.x, ..; its slab holds [policy P | value P] (cleared by the caller).
template <int D>
__global__ __launch_bounds__(256, 1) void gauss_backward_kernel(AArgs a) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *H1 = lds + L_H1 * LS, *MUZ = O + 8 * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long Pn = a.o.total;
    float *Gp = a.slab + (size_t)blockIdx.x * 2 * Pn, *Gv = Gp + Pn;
    float *scr = a.scratch + (size_t)blockIdx.x * gauss_scratch_rows(a.R) * 64;
    float *park = scr + (size_t)a3c_scratch_trunk_rows(a.R) * 64;
    const int groups = (a.n + 63) / 64;
    double lp = 0.0, lv = 0.0, ent = 0.0, wsum = 0.0;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int sbase = grp * 64, s = sbase + lane;
        const bool valid = s < a.n;
        const int ss = valid ? s : 0;
        const float wt = valid ? (a.wt ? a.wt[ss] : 1.0f) : 0.f;
        const float c = a.mult * wt, adv = a.adv[ss], cp = c * adv;
        const int len = a3c_length(a.win + (size_t)ss * a.R * D, a.R, D);
        a3c_trunk<D, D, true>(a, lds, sbase, scr);
        // ---- mu tower forward; its hidden layers (H1 and H2 are adjacent rows) wait in the scratch while the sigma tower runs
        gauss_tower_fwd<D, true>(a, lds, 0);
        if (wave < A) MUZ[wave * LS + lane] = O[wave * LS + lane];
        for (int i = wave; i < NW1 + NW2; i += 4) park[i * 64 + lane] = H1[i * LS + lane];
        __syncthreads();
        // ---- sigma tower: dz = cp * (1/sigma - d^2/sigma^3) * s (1 - s); the mu head's dz = cp * (-d/sigma^2) * 5 (1 - tanh^2)
        gauss_tower_fwd<D, true>(a, lds, 1);
        if (wave < A) {
            const float th = tanhf(MUZ[wave * LS + lane]), mu = 5.0f * th, sgm = sigmoidf_(O[wave * LS + lane]), sg = sgm + 1e-3f;
            const float d = a.raw[(size_t)ss * A + wave] - mu;
            O[wave * LS + lane] = cp * (1.0f / sg - d * d / (sg * sg * sg)) * (sgm * (1.0f - sgm));
            MUZ[wave * LS + lane] = cp * (-d / (sg * sg)) * (5.0f * (1.0f - th * th));
            if (valid && wt != 0.f) {      // weight-0 samples add nothing
                const float z = d / sg;
                lp += (double)(cp * (0.5f * z * z + logf(sg) + 0.9189385332046727f));
                ent += (double)wt * (double)(0.5f + 0.9189385332046727f + logf(sg));      // Normal entropy
                if (wave == 0) wsum += (double)wt;
            }
        }
        gauss_tower_bwd<D>(a, lds, Gp, a.o.g1w, a.o.g1b, a.o.g2w, a.o.g2b, a.o.g3w, a.o.g3b, false);
        // ---- mu tower backward on the parked layers
        for (int i = wave; i < NW1 + NW2; i += 4) H1[i * LS + lane] = park[i * 64 + lane];
        if (wave < A) O[wave * LS + lane] = MUZ[wave * LS + lane];
        gauss_tower_bwd<D>(a, lds, Gp, a.o.m1w, a.o.m1b, a.o.m2w, a.o.m2b, a.o.m3w, a.o.m3b, true);
        a3c_trunk_bwd<D, D, true>(a, lds, sbase, scr, Gp, len);
        // ---- value head
        gauss_tower_fwd<D, true>(a, lds, 2);
        if (wave == 0) {
            const float v = a.scale * O[lane], tg = a.tgt[ss], dv = v - tg;
            O[lane] = c * dv;                               // d/dz of c * 0.5 (scale z - t)^2 / scale
            if (valid) lv += (double)(c * 0.5f * dv * dv / a.scale);
        }
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
        a3c_trunk_bwd<D, D, true>(a, lds, sbase, scr, Gv, len);
    }
    // wave w < A summed action w's terms; wave 0 also the value loss
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lp += __shfl_xor(lp, d); lv += __shfl_xor(lv, d); ent += __shfl_xor(ent, d); wsum += __shfl_xor(wsum, d);
    }
    if (lane == 0 && wave < A) {
        atomicAdd(&a.stats64[0], lp);
        atomicAdd(&a.stats64[2], ent);
        if (wave == 0) { atomicAdd(&a.stats64[1], lv); atomicAdd(&a.stats64[3], wsum); }
    }
}

#include "net_gauss_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"

struct grl_anet : grl::A3cNet {
    grl_anet_config cfg;
    grl::AOff off;
    int A;                                        // actions; S0 = D = the processed observation
    // the heads' host-sample staging, rollout buffers and evaluation trace
    float *d_raw, *d_mu, *d_sigma;
    float *ro_raw, *ro_mu, *ro_sigma, *ro_act;    // ro_act (T,E,A): the action each env was stepped with
    float *ro_term_st, *ro_term_wn, *ro_term_val; // ro_term_st / ro_term_wn: always_bootstrap only
    float *term_obs;
    float *ev_act, *ev_mu;                        // ev_act (E,A): the evaluation step's actions
};

namespace grl {

static const float *anet_obs(const grl_anet *net) { return net->h->cfg.env_kind == GRL_ENV_SOLOW ? net->h->so.obs : net->h->tr.obs; }

static AArgs aargs(grl_anet *net, int n, const float *states, const float *win) {
    AArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.scale = net->cfg.scale;
    a.states = states; a.win = win; a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_anet *net, const AArgs &a) {
    if (net->D == 2) hipLaunchKernelGGL(gauss_forward_kernel<2>, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    else hipLaunchKernelGGL(gauss_forward_kernel<5>, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_anet *net, int n, const float *states, const float *win, const float *raw, const float *adv, const float *tgt,
                        const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = a3c_train_begin(net, n, gauss_scratch_rows(net->cfg.rnn_length), &blocks);
    if (rc) return rc;
    AArgs a = aargs(net, n, states, win);
    a.raw = raw; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    if (net->D == 2) hipLaunchKernelGGL(gauss_backward_kernel<2>, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    else hipLaunchKernelGGL(gauss_backward_kernel<5>, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    return a3c_train_finish(net, blocks, net->off.m1w, (double)net->A, lr0, apply, stats_host);
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_anet_config_default(grl_anet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_anet_config);
    cfg->rnn_length = 5; cfg->max_samples = 8192; cfg->lr_decay_steps = 100000; cfg->always_bootstrap = 0;
    cfg->scale = 1.f; cfg->gamma = 0.99f; cfg->gae_lambda = 0.96f; cfg->clip_norm = 40.f;
    cfg->rms_decay = 0.99f; cfg->rms_epsilon = 0.1f; cfg->lr_decay_rate = 0.96f;
    return GRL_OK;
}

int grl_anet_create(grl_handle *h, const grl_anet_config *cfg, grl_anet **out) {
    const bool solow = h && h->cfg.env_kind == GRL_ENV_SOLOW, trade = h && h->cfg.env_kind == GRL_ENV_TRADE && h->cfg.n_assets == 2;
    return a3c_create(
        "grl_anet_create", h, cfg, out,
        [&](const char *range) -> const char * {
            if (!solow && !trade) return "the Gaussian agent needs a Solow handle or a TradeAR1 handle with 2 assets";
            if (range) return range;
            if (cfg->always_bootstrap == (solow ? 1 : 0)) return nullptr;
            return solow ? "a Solow handle needs always_bootstrap = 1" : "a TradeAR1 handle needs always_bootstrap = 0";
        },
        [&](grl_anet *n, A3cGrow &Al) {
            n->S0 = n->D = solow ? 2 : 5; n->A = solow ? 1 : 2;
            n->off = gauss_offsets(n->D, n->A);
            const size_t ms = cfg->max_samples, E = h->E, A = n->A, D = n->D, W = (size_t)cfg->rnn_length * D;
            const bool ab = cfg->always_bootstrap;
            n->ro_bufs = {a3c_buf("raw", &n->ro_raw, A), a3c_buf("mu", &n->ro_mu, A), a3c_buf("sigma", &n->ro_sigma, A),
                          a3c_buf("actions", &n->ro_act, A), a3c_buf("term_values", &n->ro_term_val, 1),
                          a3c_buf("term_states", &n->ro_term_st, D, false, ab), a3c_buf("term_windows", &n->ro_term_wn, W, false, ab)};
            n->ev_bufs = {a3c_buf("mu", &n->ev_mu, A), a3c_buf("actions", &n->ev_actions, A)};
            Al(&n->d_raw, ms * A); Al(&n->d_mu, ms * A); Al(&n->d_sigma, ms * A); Al(&n->term_obs, E * D); Al(&n->ev_act, E * A);
            return (size_t)n->off.total;
        },
        {solow ? (const void *)gauss_forward_kernel<2> : (const void *)gauss_forward_kernel<5>,
         solow ? (const void *)gauss_backward_kernel<2> : (const void *)gauss_backward_kernel<5>,
         solow ? (const void *)gauss_eval_kernel<2, SolowParams> : (const void *)gauss_eval_kernel<5, TradeParams>});
}

int grl_anet_destroy(grl_anet *n) { return a3c_destroy(n); }
const char *grl_anet_last_error(const grl_anet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_anet_num_params(const grl_anet *n) { return n ? n->num_params : 0; }
int grl_anet_set_params(grl_anet *n, const float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, (float *)host, cnt, true); }
int grl_anet_get_params(grl_anet *n, float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, host, cnt, false); }
int grl_anet_get_grads(grl_anet *n, int32_t which, float *host, int64_t cnt) { return a3c_get_grads(n, "grl_anet_get_grads", which, host, cnt); }
int grl_anet_get_optimizer_state(grl_anet *n, float *msp, float *msv, int64_t cnt, int64_t *step) { return a3c_get_optimizer_state(n, msp, msv, cnt, step); }
int grl_anet_set_optimizer_state(grl_anet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) { return a3c_set_optimizer_state(n, msp, msv, cnt, step); }
int grl_anet_get_action_counter(grl_anet *n, uint64_t *out) { return a3c_get_action_counter(n, out); }
int grl_anet_set_action_counter(grl_anet *n, uint64_t v) { return a3c_set_action_counter(n, v); }
int grl_anet_set_greedy(grl_anet *net, int32_t on) { return a3c_set_greedy(net, on); }

int grl_anet_predict(grl_anet *net, int32_t n, const float *states, const float *windows, float *mu, float *sigma, float *values) {
    int rc = a3c_samples_check(net, "grl_anet_predict", n, states && windows);
    if (rc || (rc = a3c_stage(net, n, states, windows))) return rc;
    AArgs a = aargs(net, n, net->d_states, net->d_win);
    a.mu = net->d_mu; a.sigma = net->d_sigma; a.vals = net->d_vals;
    if ((rc = launch_fwd(net, a))) return rc;
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t A = net->A;
    if ((rc = a3c_get(net, mu, net->d_mu, n * A)) || (rc = a3c_get(net, sigma, net->d_sigma, n * A))) return rc;
    return a3c_get(net, values, net->d_vals, n);
}

int grl_anet_train(grl_anet *net, int32_t n, const float *states, const float *windows, const float *raw, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    int rc = a3c_samples_check(net, "grl_anet_train", n, states && windows && raw && adv && targets);
    if (rc || (rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_raw, raw, (size_t)n * net->A)) ||
        (rc = a3c_stage_targets(net, n, adv, targets, weights)))
        return rc;
    return train_device(net, n, net->d_states, net->d_win, net->d_raw, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult, lr0,
                        apply_update, stats_host);
}

int grl_anet_rollout(grl_anet *net, int32_t T) {
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, "grl_anet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = a3c_ensure_rollout(net, T);
    if (rc) return rc;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const size_t A = net->A;
    const int ab = net->cfg.always_bootstrap;
    return a3c_rollout_run(
        net, T, anet_obs(net), [&](int n, const float *states, const float *win) { return aargs(net, n, states, win); },
        [&](AArgs &a, size_t o, int t) {
            a.mu = net->ro_mu + o * A; a.sigma = net->ro_sigma + o * A;
            a.act = net->ro_act + o * A; a.raw_out = net->ro_raw + o * A; a.tanh_action = solow ? 0 : 1;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
        },
        [&](const AArgs &a) { return launch_fwd(net, a); },
        [&](size_t o) {
            return solow ? solow_launch_step(h, net->ro_act + o * A, ab ? net->term_obs : nullptr) : trade_launch_step(h, net->ro_act + o * A);
        });
}

int grl_anet_eval(grl_anet *net, int32_t max_steps, int32_t trace_steps) {
    int rc = a3c_eval_begin(net, "grl_anet_eval", max_steps, &trace_steps);
    if (rc) return rc;
    grl_handle *h = net->h;
    hipStream_t st = h->stream;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E;
    AEvalArgs v{};
    v.a = aargs(net, E, anet_obs(net), net->win);
    a3c_eval_args(net, v, max_steps, trace_steps);
    v.act = net->ev_act; v.tanh_action = solow ? 0 : 1; v.tr_mu = net->ev_mu; v.tr_act = net->ev_actions;
    if (solow) {
        SolowParams S = solow_params(h);
        hipLaunchKernelGGL((gauss_eval_kernel<2, SolowParams>), dim3((E + 63) / 64), dim3(256), A3C_LDS, st, v, S);
    } else {
        TradeParams S = trade_params(h);
        hipLaunchKernelGGL((gauss_eval_kernel<5, TradeParams>), dim3((E + 63) / 64), dim3(256), A3C_LDS, st, v, S);
    }
    return a3c_eval_finish(net, trace_steps, [&] {      // Solow: with the tape draw
        return solow ? solow_launch_reset(h, h->done_list, h->done_count, E, true) : trade_launch_reset(h, h->done_list, h->done_count, E);
    });
}

int grl_anet_read_eval(grl_anet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_anet_read_eval", which, host, bytes); }

int grl_anet_train_rollout(grl_anet *net, float lr0, float *stats_host) {
    return a3c_train_rollout(net, "grl_anet_train_rollout", [&](int n, float mult) {
        return train_device(net, n, net->ro_states, net->ro_win, net->ro_raw, net->ro_adv, net->ro_tgt, net->ro_wt, mult, lr0, 1, stats_host);
    });
}

int grl_anet_read_rollout(grl_anet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_anet_read_rollout", " exists with always_bootstrap = 1 only", which, host, bytes);
}

}  // extern "C"
