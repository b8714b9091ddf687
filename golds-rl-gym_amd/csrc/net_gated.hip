// The Ticker gated trader on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-152,338-417 and the worker loop of
// fed_gym/agents/a3c/worker.py:191-294,445-494): a GRU trunk shared by a categorical + per-choice Gaussian policy and a value
// head, the device-resident rollout on a Ticker handle and the A3C update in batched form (include/goldsrl_gatednet.h).
//
// 151 123 parameters and 163 648 MAC per sample at R = 5; the two 96 -> 256 -> 128 towers and the 96 -> 256 value layer are ~87 %
// of them, so unlike the flat GRU net this one is bound by the matrix pipe.  A workgroup of 4 waves owns 64 samples; activations
// live in LDS as [feature][sample] rows of LS = 65 floats and every dense layer is an exact-fp32 v_mfma_f32_32x32x2_f32 GEMM
// (net_mfma_gemm.inc, shared with the flat net).  The three towers run one after another through the same two buffers (256 + 128
// rows); the weights (600 KB) are read from L2.  The trunk, the LDS layout, the window rules and the update are net_a3c_core.inc,
// the host scaffold net_a3c_host.h: the Gaussian agent (net_gauss.hip) uses the same.
//   forward   one launch per rollout step: window GRU, trunk, towers, softmax / softplus, the draw and the (E,4) action write
//   backward  recomputes the forward per group (the GRU's per-step activations go to a per-workgroup scratch in global memory),
//             forms both losses' data and weight gradients and sums the weight gradients of the groups it loops over into a
//             private slab [policy P | value P]; the slabs are reduced in a fixed order (bitwise reproducible runs)
//   update    two float64 sums of squares, clip factors, both RMSProp steps -- on the device
//   eval      whole greedy episodes in one launch (net_gated_eval.inc): a workgroup keeps its 64 envs, class + normal towers only
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/goldsrl_gatednet.h"
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "ticker_dev.h"

namespace grl {

constexpr int GD = 4;         // temporal row: log prices, volumes (process_temporal_states)
constexpr int GS0 = 7;        // processed observation (TickerTraderStateProcessor); its temporal row starts at GTOFF
constexpr int GTOFF = 3;
constexpr int GNO = 12;       // normal head outputs: (asset, choice, {mu, raw sigma})
enum : uint32_t { RS_GATED_ACTION = 18 };
constexpr int A3C_DPAD = GD;
constexpr bool A3C_PAD_LAST = false;
using GS0_t = std::integral_constant<int, GS0>;      // the widths as types, for the shared per-env kernels and window rules
using GD_t = std::integral_constant<int, GD>;
using GTOFF_t = std::integral_constant<int, GTOFF>;

#include "net_a3c_core.inc"

struct GOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, c1w, c1b, c2w, c2b, c3w, c3b, n1w, n1b, n2w, n2b, n3w, n3b, v1w, v1b, v2w, v2b, total;
};

static GOff gated_offsets() {
    GOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((GD + NH) * 2 * NH); o.gb = take(2 * NH); o.cw = take((GD + NH) * NH); o.cb = take(NH);
    o.tw = take(NH * 2 * NH); o.tb = take(2 * NH); o.s1w = take(GS0 * 2 * NH); o.s1b = take(2 * NH); o.s2w = take(2 * NH * NH); o.s2b = take(NH);
    o.c1w = take(NX * NW1); o.c1b = take(NW1); o.c2w = take(NW1 * NW2); o.c2b = take(NW2); o.c3w = take(NW2 * 6); o.c3b = take(6);
    o.n1w = take(NX * NW1); o.n1b = take(NW1); o.n2w = take(NW1 * NW2); o.n2b = take(NW2); o.n3w = take(NW2 * GNO); o.n3b = take(GNO);
    o.v1w = take(NX * NW1); o.v1b = take(NW1); o.v2w = take(NW1); o.v2b = take(1);
    o.total = p;
    return o;
}

struct GArgs {
    const float *P;
    GOff o;
    int n, R;
    float scale;
    const float *states, *win;          // (n,7) (n,R,4)
    // forward outputs (any may be null)
    float *probs, *mu, *sigma, *vals;   // (n,6) (n,6) (n,6) (n)
    // acting (act != null): one sample per env
    float *act;                         // (n,4) the env's action
    int32_t *choice_out;                // (n,2)
    float *raw_out;                     // (n,2)
    uint64_t seed;
    uint32_t env_off, counter;
    int greedy;                         // the choice is the argmax, raw = mu[choice], nothing is drawn (grl_gnet_set_greedy)
    // backward
    const int32_t *choices;
    const float *raw, *adv, *tgt, *wt;  // wt may be null (all 1)
    float mult;
    float *slab;                        // [blocks][2][P]
    float *scratch;                     // [blocks][SR][64]
    double *stats64;                    // policy loss, value loss, weighted entropy sum, weight sum
};

// the shared trunk as functions of their own (not inlined, plain thread and wave index): the form these kernels were tuned in
__device__ void gated_trunk(const GArgs &a, float *lds, int sbase, float *scr) { a3c_trunk<GD, GS0, false>(a, lds, sbase, scr); }
__device__ void gated_trunk_bwd(const GArgs &a, float *lds, int sbase, const float *scr, float *G, int len) {
    a3c_trunk_bwd<GD, GS0, false>(a, lds, sbase, scr, G, len);
}

// x -> 256 ReLU -> 128 ReLU -> nout (H1, H2, O rows); tower 0 = class, 1 = normal, 2 = value (x -> 256 tanh -> 1)
__device__ void gated_tower_fwd(const GArgs &a, float *lds, int tower) {
    float *X = lds + L_X * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS, *O = lds + L_O * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = a.P;
    if (tower == 2) {
        mm_fwd(P + a.o.v1w, NW1, P + a.o.v1b, X, NX, NW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, NW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
        __syncthreads();
        return;
    }
    const long w1 = tower ? a.o.n1w : a.o.c1w, b1 = tower ? a.o.n1b : a.o.c1b, w2 = tower ? a.o.n2w : a.o.c2w,
               b2 = tower ? a.o.n2b : a.o.c2b, w3 = tower ? a.o.n3w : a.o.c3w, b3 = tower ? a.o.n3b : a.o.c3b;
    const int nout = tower ? GNO : 6;
    mm_fwd(P + w1, NW1, P + b1, X, NX, NW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, NW2, P + b2, H1, NW1, NW2, H2, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, nout, P + b3, H2, NW2, nout, O, FACT_NONE, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// softmax of one asset's 3 logits (tf.nn.softmax: exp(l - max) / sum)
__device__ __forceinline__ void softmax3(float l0, float l1, float l2, float &p0, float &p1, float &p2) {
    const float m = fmaxf(l0, fmaxf(l1, l2));
    const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
    const float z = e0 + e1 + e2;
    p0 = e0 / z; p1 = e1 / z; p2 = e2 / z;
}

// The greedy action of one asset: the first index of the largest of the three float32 probabilities (np.argmax of
// get_greedy_action, worker.py:370-372: a tie goes to the lower index), raw = mu[choice], fraction = the worker's float64 sigmoid
// (transform_raw_action, worker.py:491-494) rounded to float32.
__device__ __forceinline__ void gated_greedy_pick(float p0, float p1, float p2, float m0, float m1, float m2, int &choice, float &raw,
                                                  float &fraction) {
    int ch = p1 > p0 ? 1 : 0;
    const float best = ch ? p1 : p0;
    if (p2 > best) ch = 2;
    choice = ch;
    raw = ch == 0 ? m0 : (ch == 1 ? m1 : m2);
    fraction = (float)(1.0 / (1.0 + exp(-(double)raw)));
}

// one launch per forward pass (predict, a rollout step, the bootstrap); with a.act: the draw and the env action as well
__global__ __launch_bounds__(256) void gated_forward_kernel(GArgs a) {
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *PR = lds + L_HEAD * LS, *MU = PR + 6 * LS, *SG = MU + 6 * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane;
    const bool valid = s < a.n;
    gated_trunk(a, lds, sbase, nullptr);
    gated_tower_fwd(a, lds, 0);
    if (wave < 2) {     // wave = asset
        float p0, p1, p2;
        softmax3(O[(3 * wave) * LS + lane], O[(3 * wave + 1) * LS + lane], O[(3 * wave + 2) * LS + lane], p0, p1, p2);
        PR[(3 * wave) * LS + lane] = p0; PR[(3 * wave + 1) * LS + lane] = p1; PR[(3 * wave + 2) * LS + lane] = p2;
    }
    __syncthreads();
    gated_tower_fwd(a, lds, 1);
    for (int k = wave; k < 6; k += 4) {
        MU[k * LS + lane] = O[(2 * k) * LS + lane];
        SG[k * LS + lane] = softplusf_(O[(2 * k + 1) * LS + lane]) + 1e-7f;     // softplus + keras epsilon
    }
    __syncthreads();
    gated_tower_fwd(a, lds, 2);
    if (valid) {
        for (int k = wave; k < 6; k += 4) {
            if (a.probs) a.probs[(size_t)s * 6 + k] = PR[k * LS + lane];
            if (a.mu) a.mu[(size_t)s * 6 + k] = MU[k * LS + lane];
            if (a.sigma) a.sigma[(size_t)s * 6 + k] = SG[k * LS + lane];
        }
        if (wave == 0 && a.vals) a.vals[s] = a.scale * O[lane];
    }
    if (a.act && valid && wave < 2 && a.greedy) {
        const int as = wave;
        int ch;
        float raw, frac;
        gated_greedy_pick(PR[(3 * as) * LS + lane], PR[(3 * as + 1) * LS + lane], PR[(3 * as + 2) * LS + lane], MU[(3 * as) * LS + lane],
                          MU[(3 * as + 1) * LS + lane], MU[(3 * as + 2) * LS + lane], ch, raw, frac);
        a.choice_out[(size_t)s * 2 + as] = ch;
        a.raw_out[(size_t)s * 2 + as] = raw;
        a.act[(size_t)s * 4 + as] = (float)ch;
        a.act[(size_t)s * 4 + 2 + as] = frac;
    } else if (a.act && valid && wave < 2) {
        // get_random_discrete_action (worker.py:223-227) + get_random_action (:460-464) + transform_raw_action (:491-494)
        const int as = wave;
        double u, u1, nz, nz1;
        u01_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GATED_ACTION, 2u * as), u, u1);
        normal_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, RS_GATED_ACTION, 2u * as + 1u), nz, nz1);
        const float p0 = PR[(3 * as) * LS + lane], p1 = PR[(3 * as + 1) * LS + lane], p2 = PR[(3 * as + 2) * LS + lane];
        const float c0 = p0, c1 = c0 + p1, c2 = c1 + p2;       // float32 cumsum in index order
        const int ch = u < (double)c0 ? 0 : (u < (double)c1 ? 1 : (u < (double)c2 ? 2 : 0));
        const float raw = (float)((double)MU[(3 * as + ch) * LS + lane] + (double)SG[(3 * as + ch) * LS + lane] * nz);
        a.choice_out[(size_t)s * 2 + as] = ch;
        a.raw_out[(size_t)s * 2 + as] = raw;
        a.act[(size_t)s * 4 + as] = (float)ch;
        a.act[(size_t)s * 4 + 2 + as] = (float)(1.0 / (1.0 + exp(-(double)raw)));
    }
}

// back through a 96 -> 256 ReLU -> 128 ReLU -> nout tower whose dz of the last layer is in the O rows; d x (=|+=) into DX
__device__ void gated_tower_bwd(const GArgs &a, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, int nout,
                                bool accumulate) {
    float *X = lds + L_X * LS, *DX = lds + L_DX * LS, *H1 = lds + L_H1 * LS, *H2 = lds + L_H2 * LS, *O = lds + L_O * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = a.P;
    __syncthreads();
    mm_wgrad(H2, O, NW2, nout, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w3, NW2, nout, O, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, NW1, NW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w2, NW1, NW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, NX, NW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, NX, NW1, H1, DX, accumulate, wave, lane);
    __syncthreads();
}

// Losses (estimators.py:102-120, 377-378), per sample with coefficient c = grad_mult * weight:
//   policy  c * adv * sum_assets (-log p[choice] - log N(raw; mu_choice, sigma_choice))
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
// The workgroup loops over groups blockIdx.x, + gridDim.x, ..; its slab holds [policy P | value P] (cleared by the caller).
__global__ __launch_bounds__(256, 1) void gated_backward_kernel(GArgs a) {
    extern __shared__ float lds[];
    float *O = lds + L_O * LS, *H1 = lds + L_H1 * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
        gated_trunk(a, lds, sbase, scr);
        // ---- class tower: dz of the logits = cp * (p - onehot(choice))
        gated_tower_fwd(a, lds, 0);
        if (wave < 2) {
            const int as = wave, ch = a.choices[(size_t)ss * 2 + as];
            float p[3];
            softmax3(O[(3 * as) * LS + lane], O[(3 * as + 1) * LS + lane], O[(3 * as + 2) * LS + lane], p[0], p[1], p[2]);
            for (int k = 0; k < 3; ++k) O[(3 * as + k) * LS + lane] = cp * (p[k] - (k == ch ? 1.0f : 0.0f));
            if (valid && wt != 0.f) {      // weight-0 samples add nothing (and a 0 * log 0 would be NaN)
                const float pc = ch == 0 ? p[0] : (ch == 1 ? p[1] : p[2]);
                if (cp != 0.f) lp += (double)(cp * -logf(pc));
                float h = 0.f;
                for (int k = 0; k < 3; ++k) h -= p[k] > 0.f ? p[k] * logf(p[k]) : 0.f;
                ent += (double)wt * (double)h;
            }
        }
        gated_tower_bwd(a, lds, Gp, a.o.c1w, a.o.c1b, a.o.c2w, a.o.c2b, a.o.c3w, a.o.c3b, 6, false);
        // ---- normal tower: only the chosen (mu, sigma) of each asset gets a gradient
        gated_tower_fwd(a, lds, 1);
        if (wave < 2) {
            const int as = wave, ch = a.choices[(size_t)ss * 2 + as];
            const float mu = O[(6 * as + 2 * ch) * LS + lane], rs = O[(6 * as + 2 * ch + 1) * LS + lane];
            const float sg = softplusf_(rs) + 1e-7f, x = a.raw[(size_t)ss * 2 + as], d = x - mu;
            const float dmu = cp * (-d / (sg * sg)), dsg = cp * (1.0f / sg - d * d / (sg * sg * sg));
            for (int k = 0; k < 6; ++k) O[(6 * as + k) * LS + lane] = 0.f;
            O[(6 * as + 2 * ch) * LS + lane] = dmu;
            O[(6 * as + 2 * ch + 1) * LS + lane] = dsg * sigmoidf_(rs);
            if (valid && wt != 0.f) {
                const float z = d / sg;
                lp += (double)(cp * (0.5f * z * z + logf(sg) + 0.9189385332046727f));
                ent += (double)wt * (double)(0.5f + 0.9189385332046727f + logf(sg));      // Normal entropy
                if (as == 0) wsum += (double)wt;
            }
        }
        gated_tower_bwd(a, lds, Gp, a.o.n1w, a.o.n1b, a.o.n2w, a.o.n2b, a.o.n3w, a.o.n3b, GNO, true);
        gated_trunk_bwd(a, lds, sbase, scr, Gp, len);
        // ---- value head
        gated_tower_fwd(a, lds, 2);
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
        gated_trunk_bwd(a, lds, sbase, scr, Gv, len);
    }
    // wave w < 2 summed asset w's terms; wave 0 also the value loss
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lp += __shfl_xor(lp, d); lv += __shfl_xor(lv, d); ent += __shfl_xor(ent, d); wsum += __shfl_xor(wsum, d);
    }
    if (lane == 0 && wave < 2) {
        atomicAdd(&a.stats64[0], lp);
        atomicAdd(&a.stats64[2], ent);
        if (wave == 0) { atomicAdd(&a.stats64[1], lv); atomicAdd(&a.stats64[3], wsum); }
    }
}

__global__ void gated_boot_mask_kernel(float *__restrict__ boot, const float *__restrict__ mask, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) boot[e] = boot[e] * mask[e];      // 0 behind a finished episode (worker.py:232-237)
}

#include "net_gated_eval.inc"

}  // namespace grl


#include "net_a3c_host.h"

struct grl_gnet : grl::A3cNet {
    grl_gnet_config cfg;
    grl::GOff off;
    // the heads' host-sample staging, rollout buffers and evaluation trace
    float *d_raw, *d_probs, *d_mu, *d_sigma;
    int32_t *d_choices;
    float *ro_raw, *ro_probs, *ro_mu, *ro_sigma, *ro_act;      // ro_act (T,E,4): the action each env was stepped with
    int32_t *ro_choices;
    float *ev_probs, *ev_mu;
    int32_t *ev_choices;
};

namespace grl {

// per sample: assets (a choice and a raw draw each), (asset, choice) entries of probs / mu / sigma, the env's action
constexpr size_t GA = 2, GAC = 6, GACT = 4;

static GArgs gargs(grl_gnet *net, int n, const float *states, const float *win) {
    GArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.scale = net->cfg.scale; a.states = states; a.win = win;
    a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_gnet *net, const GArgs &a) {
    hipLaunchKernelGGL(gated_forward_kernel, dim3((a.n + 63) / 64), dim3(256), A3C_LDS, net->h->stream, a);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_gnet *net, int n, const float *states, const float *win, const int32_t *choices, const float *raw, const float *adv,
                        const float *tgt, const float *wt, float mult, float lr0, int apply, float *stats_host) {
    int blocks, rc = a3c_train_begin(net, n, a3c_scratch_trunk_rows(net->cfg.rnn_length), &blocks);
    if (rc) return rc;
    GArgs a = gargs(net, n, states, win);
    a.choices = choices; a.raw = raw; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    hipLaunchKernelGGL(gated_backward_kernel, dim3(blocks), dim3(256), A3C_LDS, net->h->stream, a);
    return a3c_train_finish(net, blocks, net->off.c1w, 2.0, lr0, apply, stats_host);
}

static int no_table(grl_gnet *net) {
    return a3c_fail(net, GRL_E_STATE, "Ticker handle has no price table yet: call grl_ticker_set_table first");
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_gnet_config_default(grl_gnet_config *cfg) {
    if (!cfg) return GRL_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(grl_gnet_config);
    cfg->rnn_length = 5; cfg->max_samples = 8192; cfg->lr_decay_steps = 100000;
    cfg->scale = 1.f; cfg->gamma = 0.99f; cfg->gae_lambda = 0.96f; cfg->clip_norm = 40.f;
    cfg->rms_decay = 0.99f; cfg->rms_epsilon = 0.1f; cfg->lr_decay_rate = 0.96f;
    return GRL_OK;
}

int grl_gnet_create(grl_handle *h, const grl_gnet_config *cfg, grl_gnet **out) {
    return a3c_create(
        "grl_gnet_create", h, cfg, out,
        [&](const char *range) { return h->cfg.env_kind != GRL_ENV_TICKER ? "the gated trader needs a Ticker handle" : range; },
        [&](grl_gnet *n, A3cGrow &Al) {
            n->S0 = GS0; n->D = GD; n->toff = GTOFF; n->off = gated_offsets();
            n->ro_bufs = {a3c_buf("raw", &n->ro_raw, GA), a3c_buf("probs", &n->ro_probs, GAC), a3c_buf("mu", &n->ro_mu, GAC),
                          a3c_buf("sigma", &n->ro_sigma, GAC), a3c_buf("choices", &n->ro_choices, GA), a3c_buf("actions", &n->ro_act, GACT)};
            n->ev_bufs = {a3c_buf("probs", &n->ev_probs, GAC), a3c_buf("mu", &n->ev_mu, GAC), a3c_buf("choices", &n->ev_choices, GA),
                          a3c_buf("actions", &n->ev_actions, GACT)};
            const size_t ms = cfg->max_samples;
            Al(&n->d_raw, ms * GA); Al(&n->d_choices, ms * GA); Al(&n->d_probs, ms * GAC); Al(&n->d_mu, ms * GAC); Al(&n->d_sigma, ms * GAC);
            return (size_t)n->off.total;
        },
        {(const void *)gated_forward_kernel, (const void *)gated_backward_kernel, (const void *)gated_eval_kernel});
}

int grl_gnet_destroy(grl_gnet *n) { return a3c_destroy(n); }
const char *grl_gnet_last_error(const grl_gnet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_gnet_num_params(const grl_gnet *n) { return n ? n->num_params : 0; }
int grl_gnet_set_params(grl_gnet *n, const float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, (float *)host, cnt, true); }
int grl_gnet_get_params(grl_gnet *n, float *host, int64_t cnt) { return a3c_copy(n, n ? n->params : nullptr, host, cnt, false); }
int grl_gnet_get_grads(grl_gnet *n, int32_t which, float *host, int64_t cnt) { return a3c_get_grads(n, "grl_gnet_get_grads", which, host, cnt); }
int grl_gnet_get_optimizer_state(grl_gnet *n, float *msp, float *msv, int64_t cnt, int64_t *step) { return a3c_get_optimizer_state(n, msp, msv, cnt, step); }
int grl_gnet_set_optimizer_state(grl_gnet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) { return a3c_set_optimizer_state(n, msp, msv, cnt, step); }
int grl_gnet_get_action_counter(grl_gnet *n, uint64_t *out) { return a3c_get_action_counter(n, out); }
int grl_gnet_set_action_counter(grl_gnet *n, uint64_t v) { return a3c_set_action_counter(n, v); }
int grl_gnet_set_greedy(grl_gnet *net, int32_t on) { return a3c_set_greedy(net, on); }

int grl_gnet_predict(grl_gnet *net, int32_t n, const float *states, const float *windows, float *probs, float *mu, float *sigma, float *values) {
    int rc = a3c_samples_check(net, "grl_gnet_predict", n, states && windows);
    if (rc || (rc = a3c_stage(net, n, states, windows))) return rc;
    GArgs a = gargs(net, n, net->d_states, net->d_win);
    a.probs = net->d_probs; a.mu = net->d_mu; a.sigma = net->d_sigma; a.vals = net->d_vals;
    if ((rc = launch_fwd(net, a))) return rc;
    A3C_HIP(net, hipStreamSynchronize(net->h->stream));
    if ((rc = a3c_get(net, probs, net->d_probs, n * GAC)) || (rc = a3c_get(net, mu, net->d_mu, n * GAC)) ||
        (rc = a3c_get(net, sigma, net->d_sigma, n * GAC)))
        return rc;
    return a3c_get(net, values, net->d_vals, n);
}

int grl_gnet_train(grl_gnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *raw,
                   const float *adv, const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update,
                   float *stats_host) {
    int rc = a3c_samples_check(net, "grl_gnet_train", n, states && windows && choices && raw && adv && targets);
    if (rc) return rc;
    for (size_t i = 0; i < n * GA; ++i)
        if (choices[i] < 0 || choices[i] > 2) return a3c_fail(net, GRL_E_INVALID, "grl_gnet_train: choices must be 0, 1 or 2");
    if ((rc = a3c_stage(net, n, states, windows)) || (rc = a3c_put(net, net->d_choices, choices, n * GA)) ||
        (rc = a3c_put(net, net->d_raw, raw, n * GA)) || (rc = a3c_stage_targets(net, n, adv, targets, weights)))
        return rc;
    return train_device(net, n, net->d_states, net->d_win, net->d_choices, net->d_raw, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr,
                        grad_mult, lr0, apply_update, stats_host);
}

int grl_gnet_rollout(grl_gnet *net, int32_t T) {
    if (!net || T < 1) return a3c_fail(net, GRL_E_INVALID, "grl_gnet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    if (!h->tk.table) return no_table(net);
    int rc = a3c_ensure_rollout(net, T);
    if (rc) return rc;
    rc = a3c_rollout_steps(
        net, T, net->cfg.rnn_length, h->tk.obs, GS0_t{}, GD_t{}, GTOFF_t{}, nullptr, nullptr, nullptr,
        [&](int n, const float *states, const float *win) { return gargs(net, n, states, win); },
        [&](GArgs &a, size_t o, int t) {
            a.probs = net->ro_probs + o * GAC; a.mu = net->ro_mu + o * GAC; a.sigma = net->ro_sigma + o * GAC;
            a.act = net->ro_act + o * GACT; a.choice_out = net->ro_choices + o * GA; a.raw_out = net->ro_raw + o * GA;
            a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
            a.greedy = net->greedy;
        },
        [&](const GArgs &a) { return launch_fwd(net, a); }, [&](size_t o) { return ticker_launch_step(h, net->ro_act + o * GACT); });
    if (rc) return rc;
    // the bootstrap is 0 behind a finished episode; then the worker's GAE (worker.py:241-294)
    const int E = h->E;
    hipLaunchKernelGGL(gated_boot_mask_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, net->ro_boot, net->ro_mask + (size_t)(T - 1) * E, E);
    if ((rc = launch_returns(h, net->ro_rew, net->ro_val, net->ro_mask, net->ro_boot, T, E, net->cfg.gamma, net->cfg.gae_lambda, net->cfg.scale,
                             0.f, 0.f, net->ro_tgt, net->ro_adv)))
        return a3c_fail(net, rc, h->err);
    A3C_HIP(net, hipGetLastError());
    return GRL_OK;
}

int grl_gnet_eval(grl_gnet *net, int32_t max_steps, int32_t trace_steps) {
    int rc = a3c_eval_begin(net, "grl_gnet_eval", max_steps, &trace_steps, [&] {
        if (!net->h->tk.table) return no_table(net);
        if (net->h->cfg.max_episode_steps < 1)
            return a3c_fail(net, GRL_E_STATE, "grl_gnet_eval: the handle has no max_episode_steps, an episode could run past its 1024-row price window");
        return (int)GRL_OK;
    });
    if (rc) return rc;
    grl_handle *h = net->h;
    const int E = h->E;
    GEvalArgs v{};
    v.a = gargs(net, E, h->tk.obs, net->win);
    a3c_eval_args(net, v, max_steps, trace_steps);
    v.tr_probs = net->ev_probs; v.tr_mu = net->ev_mu; v.tr_choices = net->ev_choices; v.tr_act = net->ev_actions;
    hipLaunchKernelGGL(gated_eval_kernel, dim3((E + 63) / 64), dim3(256), A3C_LDS, h->stream, v, ticker_params(h));
    return a3c_eval_finish(net, trace_steps, [&] { return ticker_launch_reset(h, h->done_list, h->done_count, E); });
}

int grl_gnet_read_eval(grl_gnet *net, const char *which, void *host, size_t bytes) { return a3c_read_eval(net, "grl_gnet_read_eval", which, host, bytes); }

int grl_gnet_train_rollout(grl_gnet *net, float lr0, float *stats_host) {
    return a3c_train_rollout(net, "grl_gnet_train_rollout", [&](int n, float mult) {
        return train_device(net, n, net->ro_states, net->ro_win, net->ro_choices, net->ro_raw, net->ro_adv, net->ro_tgt, net->ro_wt, mult, lr0, 1,
                            stats_host);
    });
}

int grl_gnet_read_rollout(grl_gnet *net, const char *which, void *host, size_t bytes) {
    return a3c_read_rollout(net, "grl_gnet_read_rollout", "", which, host, bytes);
}

}  // extern "C"
