// The Ticker gated trader on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-152,338-417 and the worker loop of
// fed_gym/agents/a3c/worker.py:191-294,445-494): a GRU trunk shared by a categorical + per-choice Gaussian policy and a value
// head, the device-resident rollout on a Ticker handle and the A3C update in batched form (include/goldsrl_gatednet.h).
//
// 151 123 parameters and 163 648 MAC per sample at R = 5; the two 96 -> 256 -> 128 towers and the 96 -> 256 value layer are ~87 %
// of them, so unlike the flat GRU net this one is bound by the matrix pipe.  A workgroup of 4 waves owns 64 samples; activations
// live in LDS as [feature][sample] rows of LS = 65 floats and every dense layer is an exact-fp32 v_mfma_f32_32x32x2_f32 GEMM
// (net_mfma_gemm.inc, shared with the flat net).  The three towers run one after another through the same two buffers (256 + 128
// rows); the weights (600 KB) are read from L2.
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
#include <vector>

#include "../../include/goldsrl_gatednet.h"
#include "common.h"
#include "rng.h"
#include "rollout_dev.h"
#include "ticker_dev.h"

namespace grl {

constexpr int LS = 65;        // LDS row stride
constexpr int GH = 32;        // rnn hidden
constexpr int GD = 4;         // temporal row: log prices, volumes (process_temporal_states)
constexpr int GS0 = 7;        // processed observation (TickerTraderStateProcessor)
constexpr int GX = 96;        // trunk output: [dense_temporal 64, dense_static 32]
constexpr int GW1 = 256, GW2 = 128;   // static_hidden_size * 2, static_hidden_size
constexpr int GNO = 12;       // normal head outputs: (asset, choice, {mu, raw sigma})
constexpr int GMAXR = 20;
enum : uint32_t { RS_GATED_ACTION = 18 };

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

#include "net_mfma_gemm.inc"

struct GOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, c1w, c1b, c2w, c2b, c3w, c3b, n1w, n1b, n2w, n2b, n3w, n3b, v1w, v1b, v2w, v2b, total;
};

static GOff gated_offsets() {
    GOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((GD + GH) * 2 * GH); o.gb = take(2 * GH); o.cw = take((GD + GH) * GH); o.cb = take(GH);
    o.tw = take(GH * 2 * GH); o.tb = take(2 * GH); o.s1w = take(GS0 * 2 * GH); o.s1b = take(2 * GH); o.s2w = take(2 * GH * GH); o.s2b = take(GH);
    o.c1w = take(GX * GW1); o.c1b = take(GW1); o.c2w = take(GW1 * GW2); o.c2b = take(GW2); o.c3w = take(GW2 * 6); o.c3b = take(6);
    o.n1w = take(GX * GW1); o.n1b = take(GW1); o.n2w = take(GW1 * GW2); o.n2b = take(GW2); o.n3w = take(GW2 * GNO); o.n3b = take(GNO);
    o.v1w = take(GX * GW1); o.v1b = take(GW1); o.v2w = take(GW1); o.v2b = take(1);
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

// mm_dx of net_mfma_gemm.inc written over the layer's own ReLU output: X[i][s] = X[i][s] > 0 ? dx : 0.  Every element is read and
// written by the same lane of the same tile, and the GEMM reads only W and dZ, so the dz of a ReLU layer takes no rows of its own.
__device__ __forceinline__ void mm_dx_relu_inplace(const float *__restrict__ W, int K, int N, const float *dZ, float *X, int wave, int lane) {
    const int ntiles = ((K + 31) >> 5) * 2, lr = lane & 31, kh = lane >> 5;
    for (int tile = wave; tile < ntiles; tile += 4) {
        const int i0 = (tile >> 1) * 32, s0 = (tile & 1) * 32;
        const int ia = i0 + lr, iac = ia < K ? ia : K - 1;
        f32x16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 16
        for (int k = 0; k < N; k += 2) {
            const int o = k + kh, oc = o < N ? o : N - 1;
            float av = W[(long)iac * N + oc];
            float bv = dZ[oc * LS + s0 + lr];
            av = (o < N && ia < K) ? av : 0.f;
            bv = o < N ? bv : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        const int s = s0 + lr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (i < K) X[i * LS + s] = X[i * LS + s] > 0.f ? acc[r] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------- LDS layout (rows of LS floats)
constexpr int GL_X = 0;                  // trunk output x (96)
constexpr int GL_DX = GL_X + GX;         // backward: dL/dx of the loss at hand (96)
constexpr int GL_H1 = GL_DX + GX;        // tower layer 1 (256)
constexpr int GL_H2 = GL_H1 + GW1;       // tower layer 2 (128)
constexpr int GL_O = GL_H2 + GW2;        // head outputs / their dz (16)
constexpr int GATED_LDS_ROWS = GL_O + 16;
constexpr size_t GATED_LDS = (size_t)GATED_LDS_ROWS * LS * sizeof(float);       // 154 KB: one workgroup per CU
constexpr int GL_HEAD = GL_DX;           // forward only (it has no dL/dx): probs (6), mu (6), sigma (6)
// trunk phase, inside the tower rows (free until the towers run)
constexpr int GL_HX = GL_H1;             // [x_t (4), h or r*h (32)]
constexpr int GL_HS = GL_HX + GD + GH;   // GRU state (32)
constexpr int GL_G = GL_HS + GH;         // gates r, u (64)
constexpr int GL_C = GL_G + 2 * GH;      // candidate (32)
constexpr int GL_ST = GL_C + GH;         // static input (7)
constexpr int GL_S1 = GL_ST + 8;         // dense_static 1 (64)
static_assert(GL_S1 + 2 * GH <= GL_O, "trunk rows overflow the tower rows");
// trunk backward, inside the tower rows
constexpr int GB_A = GL_H1, GB_B = GB_A + 64, GB_T = GB_B + 64, GB_DH = GB_T + 64, GB_KEEP = GB_DH + GH;
static_assert(GB_KEEP + GH <= GL_O, "trunk backward rows overflow the tower rows");

// per-workgroup scratch of the recomputed forward: per GRU step {h_prev, r, u, c} (128 rows), then h_last (32), dense_static 1 (64)
__host__ __device__ inline int gated_scratch_rows(int R) { return R * 4 * GH + GH + 2 * GH; }

// number of window rows with a non-zero entry (true_length, a3c/estimators.py:11-15)
__device__ __forceinline__ int gated_length(const float *w, int R) {
    int len = 0;
    for (int t = 0; t < R; ++t) {
        float m = 0.f;
        for (int i = 0; i < GD; ++i) m = fmaxf(m, fabsf(w[t * GD + i]));
        len += m > 0.f ? 1 : 0;
    }
    return len;
}

// rnn_graph_lstm for the group at sbase: x -> X rows.  scr != null: the GRU's per-step activations, h_last and dense_static 1 are
// kept in the workgroup's scratch for the backward.
__device__ void gated_trunk(const GArgs &a, float *lds, int sbase, float *scr) {
    float *X = lds + GL_X * LS, *HX = lds + GL_HX * LS, *HS = lds + GL_HS * LS, *G = lds + GL_G * LS, *Cc = lds + GL_C * LS,
          *ST = lds + GL_ST * LS, *S1 = lds + GL_S1 * LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = sbase + lane, ss = s < a.n ? s : 0, R = a.R;
    const float *P = a.P, *w = a.win + (size_t)ss * R * GD;
    const int len = gated_length(w, R);
    for (int i = wave; i < GH; i += 4) HS[i * LS + lane] = 0.f;
    for (int i = wave; i < GS0; i += 4) ST[i * LS + lane] = a.states[(size_t)ss * GS0 + i];
    for (int t = 0; t < R; ++t) {
        // GRUCell (TF 1.4): r,u = sigmoid([x,h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u*h + (1-u)*c
        __syncthreads();
        for (int i = wave; i < GD; i += 4) HX[i * LS + lane] = w[t * GD + i];
        for (int i = wave; i < GH; i += 4) {
            const float hv = HS[i * LS + lane];
            HX[(GD + i) * LS + lane] = hv;
            if (scr) scr[(t * 4 * GH + i) * 64 + lane] = hv;
        }
        __syncthreads();
        mm_fwd<GD + GH>(P + a.o.gw, 2 * GH, P + a.o.gb, HX, GD + GH, 2 * GH, G, FACT_SIGMOID, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < GH; i += 4) HX[(GD + i) * LS + lane] = G[i * LS + lane] * HS[i * LS + lane];
        __syncthreads();
        mm_fwd<GD + GH>(P + a.o.cw, GH, P + a.o.cb, HX, GD + GH, GH, Cc, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < GH; i += 4) {
            const float u = G[(GH + i) * LS + lane], c = Cc[i * LS + lane];
            if (scr) {
                scr[(t * 4 * GH + GH + i) * 64 + lane] = G[i * LS + lane];
                scr[(t * 4 * GH + 2 * GH + i) * 64 + lane] = u;
                scr[(t * 4 * GH + 3 * GH + i) * 64 + lane] = c;
            }
            if (t < len) HS[i * LS + lane] = u * HS[i * LS + lane] + (1.0f - u) * c;   // dynamic_rnn(sequence_length)
        }
    }
    __syncthreads();
    if (scr)
        for (int i = wave; i < GH; i += 4) scr[(R * 4 * GH + i) * 64 + lane] = HS[i * LS + lane];
    mm_fwd(P + a.o.tw, 2 * GH, P + a.o.tb, HS, GH, 2 * GH, X, FACT_RELU, nullptr, 0, 0, wave, lane);
    mm_fwd(P + a.o.s1w, 2 * GH, P + a.o.s1b, ST, GS0, 2 * GH, S1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    if (scr)
        for (int i = wave; i < 2 * GH; i += 4) scr[(R * 4 * GH + GH + i) * 64 + lane] = S1[i * LS + lane];
    mm_fwd(P + a.o.s2w, GH, P + a.o.s2b, S1, 2 * GH, GH, X + 2 * GH * LS, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// x -> 256 ReLU -> 128 ReLU -> nout (H1, H2, O rows); tower 0 = class, 1 = normal, 2 = value (x -> 256 tanh -> 1)
__device__ void gated_tower_fwd(const GArgs &a, float *lds, int tower) {
    float *X = lds + GL_X * LS, *H1 = lds + GL_H1 * LS, *H2 = lds + GL_H2 * LS, *O = lds + GL_O * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = a.P;
    if (tower == 2) {
        mm_fwd(P + a.o.v1w, GW1, P + a.o.v1b, X, GX, GW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, GW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
        __syncthreads();
        return;
    }
    const long w1 = tower ? a.o.n1w : a.o.c1w, b1 = tower ? a.o.n1b : a.o.c1b, w2 = tower ? a.o.n2w : a.o.c2w,
               b2 = tower ? a.o.n2b : a.o.c2b, w3 = tower ? a.o.n3w : a.o.c3w, b3 = tower ? a.o.n3b : a.o.c3b;
    const int nout = tower ? GNO : 6;
    mm_fwd(P + w1, GW1, P + b1, X, GX, GW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, GW2, P + b2, H1, GW1, GW2, H2, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, nout, P + b3, H2, GW2, nout, O, FACT_NONE, nullptr, 0, 0, wave, lane);
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
    float *O = lds + GL_O * LS, *PR = lds + GL_HEAD * LS, *MU = PR + 6 * LS, *SG = MU + 6 * LS;
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

// trunk backward for one loss: DX rows hold dL/dx; weight gradients go to G (a slab half)
__device__ void gated_trunk_bwd(const GArgs &a, float *lds, int sbase, const float *scr, float *G, int len) {
    float *X = lds + GL_X * LS, *DX = lds + GL_DX * LS, *BA = lds + GB_A * LS, *BB = lds + GB_B * LS, *BT = lds + GB_T * LS,
          *DH = lds + GB_DH * LS, *KEEP = lds + GB_KEEP * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = sbase + lane, ss = s < a.n ? s : 0, R = a.R;
    const float *P = a.P, *w = a.win + (size_t)ss * R * GD;
    auto S = [&](int f) { return scr[f * 64 + lane]; };
    __syncthreads();
    // static path: x[64..96) = relu(S1 W2 + b2), S1 = relu(states W1 + b1)
    for (int i = wave; i < GH; i += 4) BB[i * LS + lane] = X[(2 * GH + i) * LS + lane] > 0.f ? DX[(2 * GH + i) * LS + lane] : 0.f;
    for (int i = wave; i < 2 * GH; i += 4) BA[i * LS + lane] = S(R * 4 * GH + GH + i);
    __syncthreads();
    mm_wgrad(BA, BB, 2 * GH, GH, G + a.o.s2w, G + a.o.s2b, wave, lane);
    mm_dx(P + a.o.s2w, 2 * GH, GH, BB, BT, false, wave, lane);
    __syncthreads();
    for (int i = wave; i < 2 * GH; i += 4) BB[i * LS + lane] = BA[i * LS + lane] > 0.f ? BT[i * LS + lane] : 0.f;
    __syncthreads();
    for (int i = wave; i < GS0; i += 4) BA[i * LS + lane] = a.states[(size_t)ss * GS0 + i];
    __syncthreads();
    mm_wgrad(BA, BB, GS0, 2 * GH, G + a.o.s1w, G + a.o.s1b, wave, lane);
    __syncthreads();
    // dense_temporal
    for (int i = wave; i < 2 * GH; i += 4) BB[i * LS + lane] = X[i * LS + lane] > 0.f ? DX[i * LS + lane] : 0.f;
    for (int i = wave; i < GH; i += 4) BA[i * LS + lane] = S(R * 4 * GH + i);
    __syncthreads();
    mm_wgrad(BA, BB, GH, 2 * GH, G + a.o.tw, G + a.o.tb, wave, lane);
    mm_dx(P + a.o.tw, GH, 2 * GH, BB, DH, false, wave, lane);
    // GRU, back through time with the sequence-length mask
    for (int t = R - 1; t >= 0; --t) {
        const bool act = t < len;
        __syncthreads();
        for (int i = wave; i < GD; i += 4) BA[i * LS + lane] = w[t * GD + i];
        for (int i = wave; i < GH; i += 4) {
            const int f = t * 4 * GH;
            const float hp = S(f + i), r = S(f + GH + i), u = S(f + 2 * GH + i), c = S(f + 3 * GH + i);
            const float dhn = act ? DH[i * LS + lane] : 0.f;
            KEEP[i * LS + lane] = dhn * u;
            BB[i * LS + lane] = dhn * (1.0f - u) * (1.0f - c * c);             // dz of the candidate
            BB[(GH + i) * LS + lane] = dhn * (hp - c) * u * (1.0f - u);         // dz of the update gate (kept for later)
            BA[(GD + i) * LS + lane] = r * hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, GD + GH, GH, G + a.o.cw, G + a.o.cb, wave, lane);
        mm_dx(P + a.o.cw, GD + GH, GH, BB, BT, false, wave, lane);
        __syncthreads();
        for (int i = wave; i < GH; i += 4) {
            const int f = t * 4 * GH;
            const float hp = S(f + i), r = S(f + GH + i);
            const float drh = BT[(GD + i) * LS + lane];
            KEEP[i * LS + lane] += drh * r;
            BB[i * LS + lane] = drh * hp * r * (1.0f - r);                     // dz of the reset gate
            BA[(GD + i) * LS + lane] = hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, GD + GH, 2 * GH, G + a.o.gw, G + a.o.gb, wave, lane);
        mm_dx(P + a.o.gw, GD + GH, 2 * GH, BB, BT, false, wave, lane);
        __syncthreads();
        if (act)
            for (int i = wave; i < GH; i += 4) DH[i * LS + lane] = KEEP[i * LS + lane] + BT[(GD + i) * LS + lane];
    }
    __syncthreads();
}

// back through a 96 -> 256 ReLU -> 128 ReLU -> nout tower whose dz of the last layer is in the O rows; d x (=|+=) into DX
__device__ void gated_tower_bwd(const GArgs &a, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, int nout,
                                bool accumulate) {
    float *X = lds + GL_X * LS, *DX = lds + GL_DX * LS, *H1 = lds + GL_H1 * LS, *H2 = lds + GL_H2 * LS, *O = lds + GL_O * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = a.P;
    __syncthreads();
    mm_wgrad(H2, O, GW2, nout, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_relu_inplace(P + w3, GW2, nout, O, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, GW1, GW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_relu_inplace(P + w2, GW1, GW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, GX, GW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, GX, GW1, H1, DX, accumulate, wave, lane);
    __syncthreads();
}

// Losses (estimators.py:102-120, 377-378), per sample with coefficient c = grad_mult * weight:
//   policy  c * adv * sum_assets (-log p[choice] - log N(raw; mu_choice, sigma_choice))
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
// The workgroup loops over groups blockIdx.x, + gridDim.x, ..; its slab holds [policy P | value P] (cleared by the caller).
__global__ __launch_bounds__(256, 1) void gated_backward_kernel(GArgs a) {
    extern __shared__ float lds[];
    float *O = lds + GL_O * LS, *H1 = lds + GL_H1 * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long Pn = a.o.total;
    float *Gp = a.slab + (size_t)blockIdx.x * 2 * Pn, *Gv = Gp + Pn;
    float *scr = a.scratch + (size_t)blockIdx.x * gated_scratch_rows(a.R) * 64;
    const int groups = (a.n + 63) / 64;
    double lp = 0.0, lv = 0.0, ent = 0.0, wsum = 0.0;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int sbase = grp * 64, s = sbase + lane;
        const bool valid = s < a.n;
        const int ss = valid ? s : 0;
        const float wt = valid ? (a.wt ? a.wt[ss] : 1.0f) : 0.f;
        const float c = a.mult * wt, adv = a.adv[ss], cp = c * adv;
        const int len = gated_length(a.win + (size_t)ss * a.R * GD, a.R);
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
        mm_wgrad(H1, O, GW1, 1, Gv + a.o.v2w, Gv + a.o.v2b, wave, lane);
        __syncthreads();
        for (int i = wave; i < GW1; i += 4) {
            const float h = H1[i * LS + lane];
            H1[i * LS + lane] = a.P[a.o.v2w + i] * O[lane] * (1.0f - h * h);
        }
        __syncthreads();
        mm_wgrad(lds + GL_X * LS, H1, GX, GW1, Gv + a.o.v1w, Gv + a.o.v1b, wave, lane);
        mm_dx(a.P + a.o.v1w, GX, GW1, H1, lds + GL_DX * LS, false, wave, lane);
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

#include "net_a3c_update.inc"

// ---------------------------------------------------------------------------------------------- rollout
// window of env e: rows [0, min(k+1, R)) hold the episode's last temporal rows (current last), zero rows after; k = kstep[e]
__device__ __forceinline__ void gated_window_restart(float *win, int R, const float *obs) {
    for (int i = 0; i < GD; ++i) win[i] = obs[3 + i];
    for (int i = GD; i < R * GD; ++i) win[i] = 0.f;
}

// after the env step: the window restarts on done (o is the reset observation) or takes the new row; returns the env's new k
__device__ __forceinline__ int gated_window_step(float *w, int R, int k, bool done, const float *o) {
    if (done) { gated_window_restart(w, R, o); return 0; }
    k += 1;
    if (k < R) {
        for (int i = 0; i < GD; ++i) w[k * GD + i] = o[3 + i];
    } else {
        for (int i = 0; i < (R - 1) * GD; ++i) w[i] = w[i + GD];
        for (int i = 0; i < GD; ++i) w[(R - 1) * GD + i] = o[3 + i];
    }
    return k;
}

// before a rollout: envs the handle (re)set since (elapsed 0), or all of them the first time, start a new window
__global__ void gated_sync_kernel(const int32_t *__restrict__ elapsed, const float *__restrict__ obs, float *__restrict__ win,
                                  int32_t *__restrict__ kstep, int E, int R, int all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (all || elapsed[e] == 0) {
        gated_window_restart(win + (size_t)e * R * GD, R, obs + (size_t)e * GS0);
        kstep[e] = 0;
    }
}

// record the step's inputs: states[t], windows[t], weights[t] (the worker records a transition once its history has R rows)
__global__ void gated_record_kernel(const float *__restrict__ obs, const float *__restrict__ win, const int32_t *__restrict__ kstep, int E,
                                    int R, float *__restrict__ st, float *__restrict__ wn, float *__restrict__ wt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    for (int i = 0; i < GS0; ++i) st[(size_t)e * GS0 + i] = obs[(size_t)e * GS0 + i];
    for (int i = 0; i < R * GD; ++i) wn[(size_t)e * R * GD + i] = win[(size_t)e * R * GD + i];
    if (wt) wt[e] = kstep[e] >= R - 1 ? 1.0f : 0.0f;
}

// after the env step: reward, done, mask; the window restarts on done (the observation is the reset one) or takes the new row
__global__ void gated_post_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done, const float *__restrict__ obs,
                                  float *__restrict__ win, int32_t *__restrict__ kstep, int E, int R, float *__restrict__ rew,
                                  float *__restrict__ dn, float *__restrict__ mask) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool d = done[e] != 0;
    rew[e] = reward[e];
    dn[e] = d ? 1.0f : 0.0f;
    mask[e] = d ? 0.0f : 1.0f;
    kstep[e] = gated_window_step(win + (size_t)e * R * GD, R, kstep[e], d, obs + (size_t)e * GS0);
}

__global__ void gated_boot_mask_kernel(float *__restrict__ boot, const float *__restrict__ mask, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) boot[e] = boot[e] * mask[e];      // 0 behind a finished episode (worker.py:232-237)
}

#include "net_gated_eval.inc"

}  // namespace grl

struct grl_gnet {
    grl_handle *h;
    grl_gnet_config cfg;
    std::string err;
    grl::GOff off;
    float *params, *grads, *msp, *msv, *stats;    // grads: [policy P | value P]
    double *stats64;                              // 4 loss sums, then 2 x kA3cSumsqBlocks partial sums
    int64_t global_step;
    uint64_t act_counter;
    int greedy;                                   // grl_gnet_set_greedy
    // host-sample staging
    float *d_states, *d_win, *d_raw, *d_adv, *d_tgt, *d_wt, *d_probs, *d_mu, *d_sigma, *d_vals;
    int32_t *d_choices;
    // training workspace (grown on demand)
    float *slab, *scratch;
    int ws_blocks;
    // rollout
    float *win;                                   // (E,R,4) each env's current window
    int32_t *kstep;
    int win_init;
    int T;
    float *ro_states, *ro_win, *ro_raw, *ro_probs, *ro_mu, *ro_sigma, *ro_val, *ro_rew, *ro_done, *ro_mask, *ro_wt, *ro_adv, *ro_tgt;
    float *ro_boot, *ro_act, *boot_states, *boot_win;      // ro_act (T,E,4): the action each env was stepped with
    int32_t *ro_choices;
    // grl_gnet_eval: per-env results and the trace of the first ev_trace steps
    double *ev_total;
    int32_t *ev_len;
    uint8_t *ev_fin;
    float *ev_states, *ev_probs, *ev_mu, *ev_actions, *ev_rew, *ev_done;
    int32_t *ev_choices;
    int32_t ev_reset_count;                       // E, the source of the reset list's count (outlives the async copy)
    int ev_trace, ev_trace_cap, ev_played;        // ev_played: -1 until grl_gnet_read_eval has looked, -2 before any evaluation
    std::vector<void *> allocs, ro_allocs, ws_allocs, ev_allocs;
};

namespace grl {

static int gfail(grl_gnet *n, int code, const std::string &msg) {
    if (n) n->err = msg;
    return code;
}
#define GNET_HIP(n, call)                                                                                  \
    do {                                                                                                   \
        hipError_t _e = (call);                                                                            \
        if (_e != hipSuccess) return gfail(n, GRL_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
static int galloc(grl_gnet *n, T **p, size_t count, std::vector<void *> &list) {
    GNET_HIP(n, hipMalloc((void **)p, (count ? count : 1) * sizeof(T)));
    list.push_back(*p);
    GNET_HIP(n, hipMemsetAsync(*p, 0, (count ? count : 1) * sizeof(T), n->h->stream));
    return GRL_OK;
}

static GArgs gargs(grl_gnet *net, int n, const float *states, const float *win) {
    GArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.scale = net->cfg.scale; a.states = states; a.win = win;
    a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_gnet *net, const GArgs &a) {
    hipLaunchKernelGGL(gated_forward_kernel, dim3((a.n + 63) / 64), dim3(256), GATED_LDS, net->h->stream, a);
    GNET_HIP(net, hipGetLastError());
    return GRL_OK;
}

// the backward's slabs and scratch for `blocks` workgroups
static int ensure_ws(grl_gnet *net, int blocks) {
    if (blocks <= net->ws_blocks) return GRL_OK;
    GNET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ws_allocs) hipFree(p);
    net->ws_allocs.clear();
    net->ws_blocks = 0;
    int rc = galloc(net, &net->slab, (size_t)blocks * 2 * net->off.total, net->ws_allocs);
    if (!rc) rc = galloc(net, &net->scratch, (size_t)blocks * gated_scratch_rows(net->cfg.rnn_length) * 64, net->ws_allocs);
    if (!rc) net->ws_blocks = blocks;
    return rc;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_gnet *net, int n, const float *states, const float *win, const int32_t *choices, const float *raw, const float *adv,
                        const float *tgt, const float *wt, float mult, float lr0, int apply, float *stats_host) {
    hipStream_t st = net->h->stream;
    const int groups = (n + 63) / 64, blocks = groups < 256 ? groups : 256;      // 154 KB of LDS: one workgroup per CU
    int rc = ensure_ws(net, blocks);
    if (rc) return rc;
    const long P = net->off.total;
    GNET_HIP(net, hipMemsetAsync(net->slab, 0, (size_t)blocks * 2 * P * sizeof(float), st));
    GNET_HIP(net, hipMemsetAsync(net->stats64, 0, 4 * sizeof(double), st));
    GArgs a = gargs(net, n, states, win);
    a.choices = choices; a.raw = raw; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    hipLaunchKernelGGL(gated_backward_kernel, dim3(blocks), dim3(256), GATED_LDS, st, a);
    hipLaunchKernelGGL(flat_slab_reduce_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(1024), 0, st, net->slab, blocks, 2 * P, net->grads);
    hipLaunchKernelGGL(a3c_sumsq_kernel, dim3(kA3cSumsqBlocks, 2), dim3(256), 0, st, net->grads, P, net->stats64 + 4);
    // tf.train.exponential_decay(lr0, global_step, decay_steps, rate, staircase=False), global_step before the update
    const float lr = (float)((double)lr0 * pow((double)net->cfg.lr_decay_rate, (double)net->global_step / (double)net->cfg.lr_decay_steps));
    hipLaunchKernelGGL(a3c_finalize_kernel, dim3(1), dim3(64), 0, st, net->stats64, net->stats64 + 4, 2.0, net->cfg.clip_norm, lr, net->stats);
    if (apply) {
        hipLaunchKernelGGL(a3c_rmsprop_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, net->params, net->grads, net->msp, net->msv, P,
                           net->off.c1w, net->off.v1w, net->stats, net->cfg.rms_decay, net->cfg.rms_epsilon);
        net->global_step += 2;      // both train ops increment it (estimators.py:137-140, 403-406)
    }
    GNET_HIP(net, hipGetLastError());
    GNET_HIP(net, hipStreamSynchronize(st));
    if (stats_host) {
        float s[6];
        GNET_HIP(net, hipMemcpy(s, net->stats, sizeof(s), hipMemcpyDeviceToHost));
        for (int i = 0; i < 6; ++i) stats_host[i] = s[i];
    }
    return GRL_OK;
}

static int ensure_rollout(grl_gnet *net, int T) {
    if (T == net->T) return GRL_OK;
    GNET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ro_allocs) hipFree(p);
    net->ro_allocs.clear();
    net->T = 0;
    const size_t E = net->h->E, R = net->cfg.rnn_length, TE = (size_t)T * E;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = galloc(net, p, cnt, net->ro_allocs); };
    Al(&net->ro_states, TE * GS0); Al(&net->ro_win, TE * R * GD); Al(&net->ro_raw, TE * 2); Al(&net->ro_probs, TE * 6);
    Al(&net->ro_mu, TE * 6); Al(&net->ro_sigma, TE * 6); Al(&net->ro_val, TE); Al(&net->ro_rew, TE); Al(&net->ro_done, TE);
    Al(&net->ro_mask, TE); Al(&net->ro_wt, TE); Al(&net->ro_adv, TE); Al(&net->ro_tgt, TE); Al(&net->ro_act, TE * 4);
    if (rc == GRL_OK) rc = galloc(net, &net->ro_choices, TE * 2, net->ro_allocs);
    if (rc == GRL_OK) net->T = T;
    return rc;
}

// the trace buffers of grl_gnet_eval for `steps` steps (they only grow)
static int ensure_eval_trace(grl_gnet *net, int steps) {
    if (steps <= net->ev_trace_cap) return GRL_OK;
    GNET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ev_allocs) hipFree(p);
    net->ev_allocs.clear();
    net->ev_trace_cap = -1;
    const size_t SE = (size_t)steps * net->h->E;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = galloc(net, p, cnt, net->ev_allocs); };
    Al(&net->ev_states, SE * GS0); Al(&net->ev_probs, SE * 6); Al(&net->ev_mu, SE * 6); Al(&net->ev_actions, SE * 4); Al(&net->ev_rew, SE);
    Al(&net->ev_done, SE);
    if (rc == GRL_OK) rc = galloc(net, &net->ev_choices, SE * 2, net->ev_allocs);
    if (rc == GRL_OK) net->ev_trace_cap = steps;
    return rc;
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
    if (!h || !cfg || !out) return GRL_E_INVALID;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(grl_gnet_config)) return fail(h, GRL_E_INVALID, "grl_gnet_create: config size mismatch");
    if (h->cfg.env_kind != GRL_ENV_TICKER) return fail(h, GRL_E_INVALID, "grl_gnet_create: the gated trader needs a Ticker handle");
    if (cfg->rnn_length < 1 || cfg->rnn_length > GMAXR || cfg->max_samples < 1 || cfg->lr_decay_steps < 1 || !(cfg->scale != 0.f) ||
        !(cfg->gae_lambda > 0.f && cfg->gae_lambda <= 1.f))
        return fail(h, GRL_E_INVALID, "grl_gnet_create: config out of range (rnn_length 1..20)");
    hipSetDevice(h->cfg.device_id);
    grl_gnet *n = new grl_gnet();
    n->h = h; n->cfg = *cfg; n->off = gated_offsets();
    n->global_step = 0; n->act_counter = 0; n->greedy = 0; n->ws_blocks = 0; n->win_init = 0; n->T = 0;
    n->ev_trace = 0; n->ev_trace_cap = -1; n->ev_played = -2;
    const size_t ms = cfg->max_samples, P = n->off.total, R = cfg->rnn_length, E = h->E;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = galloc(n, p, cnt, n->allocs); };
    Al(&n->params, P); Al(&n->grads, 2 * P); Al(&n->msp, P); Al(&n->msv, P); Al(&n->stats, 8);
    Al(&n->d_states, ms * GS0); Al(&n->d_win, ms * R * GD); Al(&n->d_raw, ms * 2); Al(&n->d_adv, ms); Al(&n->d_tgt, ms); Al(&n->d_wt, ms);
    Al(&n->d_probs, ms * 6); Al(&n->d_mu, ms * 6); Al(&n->d_sigma, ms * 6); Al(&n->d_vals, ms);
    Al(&n->win, E * R * GD); Al(&n->ro_boot, E); Al(&n->boot_states, E * GS0); Al(&n->boot_win, E * R * GD);
    if (rc == GRL_OK) rc = galloc(n, &n->d_choices, ms * 2, n->allocs);
    if (rc == GRL_OK) rc = galloc(n, &n->kstep, E, n->allocs);
    if (rc == GRL_OK) rc = galloc(n, &n->stats64, 4 + 2 * kA3cSumsqBlocks, n->allocs);
    if (rc == GRL_OK) rc = galloc(n, &n->ev_total, E, n->allocs);
    if (rc == GRL_OK) rc = galloc(n, &n->ev_len, E, n->allocs);
    if (rc == GRL_OK) rc = galloc(n, &n->ev_fin, E, n->allocs);
    if (rc == GRL_OK) {      // RMSProp ms starts at ones (TF 1.x)
        hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, n->msp, (long)P, 1.0f);
        hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, n->msv, (long)P, 1.0f);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)gated_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GATED_LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)gated_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GATED_LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)gated_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GATED_LDS);
        if (e != hipSuccess) rc = gfail(n, GRL_E_HIP, std::string("grl_gnet_create: ") + hipGetErrorString(e));
    }
    if (rc != GRL_OK) {
        fail(h, rc, "grl_gnet_create: " + n->err);
        grl_gnet_destroy(n);
        return rc;
    }
    hipStreamSynchronize(h->stream);
    *out = n;
    return GRL_OK;
}

int grl_gnet_destroy(grl_gnet *n) {
    if (!n) return GRL_OK;
    grl_sync_for_destroy(n->h);
    for (void *p : n->allocs) hipFree(p);
    for (void *p : n->ro_allocs) hipFree(p);
    for (void *p : n->ws_allocs) hipFree(p);
    for (void *p : n->ev_allocs) hipFree(p);
    delete n;
    return GRL_OK;
}

const char *grl_gnet_last_error(const grl_gnet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_gnet_num_params(const grl_gnet *n) { return n ? n->off.total : 0; }

static int gcopy(grl_gnet *n, float *dev, float *host, int64_t cnt, int64_t want, bool to_dev) {
    if (!n || !host) return gfail(n, GRL_E_INVALID, "null argument");
    if (cnt != want) return gfail(n, GRL_E_SIZE, "length must be num_params");
    hipSetDevice(n->h->cfg.device_id);
    GNET_HIP(n, hipStreamSynchronize(n->h->stream));
    GNET_HIP(n, hipMemcpy(to_dev ? (void *)dev : (void *)host, to_dev ? (const void *)host : (const void *)dev, (size_t)cnt * 4,
                          to_dev ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_gnet_set_params(grl_gnet *n, const float *host, int64_t cnt) { return gcopy(n, n ? n->params : nullptr, (float *)host, cnt, n ? n->off.total : 0, true); }
int grl_gnet_get_params(grl_gnet *n, float *host, int64_t cnt) { return gcopy(n, n ? n->params : nullptr, host, cnt, n ? n->off.total : 0, false); }
int grl_gnet_get_grads(grl_gnet *n, int32_t which, float *host, int64_t cnt) {
    if (n && which != GRL_GNET_POLICY && which != GRL_GNET_VALUE) return gfail(n, GRL_E_INVALID, "grl_gnet_get_grads: which is 0 or 1");
    return gcopy(n, n ? n->grads + (which ? n->off.total : 0) : nullptr, host, cnt, n ? n->off.total : 0, false);
}

int grl_gnet_get_optimizer_state(grl_gnet *n, float *msp, float *msv, int64_t cnt, int64_t *step) {
    int rc = gcopy(n, n ? n->msp : nullptr, msp, cnt, n ? n->off.total : 0, false);
    if (!rc) rc = gcopy(n, n->msv, msv, cnt, n->off.total, false);
    if (!rc && step) *step = n->global_step;
    return rc;
}

int grl_gnet_set_optimizer_state(grl_gnet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) {
    if (n && step < 0) return gfail(n, GRL_E_INVALID, "global step must be >= 0");
    int rc = gcopy(n, n ? n->msp : nullptr, (float *)msp, cnt, n ? n->off.total : 0, true);
    if (!rc) rc = gcopy(n, n->msv, (float *)msv, cnt, n->off.total, true);
    if (!rc) n->global_step = step;
    return rc;
}

int grl_gnet_get_action_counter(grl_gnet *n, uint64_t *out) {
    if (!n || !out) return GRL_E_INVALID;
    *out = n->act_counter;
    return GRL_OK;
}

int grl_gnet_set_action_counter(grl_gnet *n, uint64_t v) {
    if (!n) return GRL_E_INVALID;
    n->act_counter = v;
    return GRL_OK;
}

int grl_gnet_predict(grl_gnet *net, int32_t n, const float *states, const float *windows, float *probs, float *mu, float *sigma, float *values) {
    if (!net || n <= 0 || !states || !windows) return gfail(net, GRL_E_INVALID, "grl_gnet_predict: bad argument");
    if (n > net->cfg.max_samples) return gfail(net, GRL_E_SIZE, "grl_gnet_predict: n exceeds max_samples");
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    const size_t R = net->cfg.rnn_length;
    GNET_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * GS0 * 4, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_win, windows, (size_t)n * R * GD * 4, hipMemcpyHostToDevice, st));
    GArgs a = gargs(net, n, net->d_states, net->d_win);
    a.probs = net->d_probs; a.mu = net->d_mu; a.sigma = net->d_sigma; a.vals = net->d_vals;
    int rc = launch_fwd(net, a);
    if (rc) return rc;
    GNET_HIP(net, hipStreamSynchronize(st));
    if (probs) GNET_HIP(net, hipMemcpy(probs, net->d_probs, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (mu) GNET_HIP(net, hipMemcpy(mu, net->d_mu, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (sigma) GNET_HIP(net, hipMemcpy(sigma, net->d_sigma, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (values) GNET_HIP(net, hipMemcpy(values, net->d_vals, (size_t)n * 4, hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_gnet_train(grl_gnet *net, int32_t n, const float *states, const float *windows, const int32_t *choices, const float *raw,
                   const float *adv, const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update,
                   float *stats_host) {
    if (!net || n <= 0 || !states || !windows || !choices || !raw || !adv || !targets) return gfail(net, GRL_E_INVALID, "grl_gnet_train: bad argument");
    if (n > net->cfg.max_samples) return gfail(net, GRL_E_SIZE, "grl_gnet_train: n exceeds max_samples");
    for (int i = 0; i < 2 * n; ++i)
        if (choices[i] < 0 || choices[i] > 2) return gfail(net, GRL_E_INVALID, "grl_gnet_train: choices must be 0, 1 or 2");
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    const size_t R = net->cfg.rnn_length;
    GNET_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * GS0 * 4, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_win, windows, (size_t)n * R * GD * 4, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_choices, choices, (size_t)n * 8, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_raw, raw, (size_t)n * 8, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_adv, adv, (size_t)n * 4, hipMemcpyHostToDevice, st));
    GNET_HIP(net, hipMemcpyAsync(net->d_tgt, targets, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (weights) GNET_HIP(net, hipMemcpyAsync(net->d_wt, weights, (size_t)n * 4, hipMemcpyHostToDevice, st));
    return train_device(net, n, net->d_states, net->d_win, net->d_choices, net->d_raw, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr,
                        grad_mult, lr0, apply_update, stats_host);
}

int grl_gnet_rollout(grl_gnet *net, int32_t T) {
    if (!net || T < 1) return gfail(net, GRL_E_INVALID, "grl_gnet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    if (!h->tk.table) return gfail(net, GRL_E_STATE, "Ticker handle has no price table yet: call grl_ticker_set_table first");
    int rc = ensure_rollout(net, T);
    if (rc) return rc;
    hipStream_t st = h->stream;
    const int E = h->E, R = net->cfg.rnn_length, eb = (E + 255) / 256;
    hipLaunchKernelGGL(gated_sync_kernel, dim3(eb), dim3(256), 0, st, h->elapsed, h->tk.obs, net->win, net->kstep, E, R, net->win_init ? 0 : 1);
    net->win_init = 1;
    for (int t = 0; t < T; ++t) {
        const size_t o = (size_t)t * E;
        hipLaunchKernelGGL(gated_record_kernel, dim3(eb), dim3(256), 0, st, h->tk.obs, net->win, net->kstep, E, R, net->ro_states + o * GS0,
                           net->ro_win + o * R * GD, net->ro_wt + o);
        GArgs a = gargs(net, E, net->ro_states + o * GS0, net->ro_win + o * R * GD);
        a.probs = net->ro_probs + o * 6; a.mu = net->ro_mu + o * 6; a.sigma = net->ro_sigma + o * 6; a.vals = net->ro_val + o;
        a.act = net->ro_act + o * 4; a.choice_out = net->ro_choices + o * 2; a.raw_out = net->ro_raw + o * 2;
        a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
        a.greedy = net->greedy;
        if ((rc = launch_fwd(net, a))) return rc;
        if ((rc = ticker_launch_step(h, net->ro_act + o * 4))) return gfail(net, rc, h->err);
        if ((rc = episodes_launch_account(h))) return gfail(net, rc, h->err);
        hipLaunchKernelGGL(gated_post_kernel, dim3(eb), dim3(256), 0, st, h->reward, h->done, h->tk.obs, net->win, net->kstep, E, R,
                           net->ro_rew + o, net->ro_done + o, net->ro_mask + o);
    }
    if (!net->greedy) net->act_counter += (uint64_t)T;      // a greedy rollout draws nothing
    // bootstrap: V of the window after the last step, 0 behind a finished episode; then the worker's GAE (worker.py:241-294)
    hipLaunchKernelGGL(gated_record_kernel, dim3(eb), dim3(256), 0, st, h->tk.obs, net->win, net->kstep, E, R, net->boot_states, net->boot_win,
                       (float *)nullptr);
    GArgs b = gargs(net, E, net->boot_states, net->boot_win);
    b.vals = net->ro_boot;
    if ((rc = launch_fwd(net, b))) return rc;
    hipLaunchKernelGGL(gated_boot_mask_kernel, dim3(eb), dim3(256), 0, st, net->ro_boot, net->ro_mask + (size_t)(T - 1) * E, E);
    if ((rc = launch_returns(h, net->ro_rew, net->ro_val, net->ro_mask, net->ro_boot, T, E, net->cfg.gamma, net->cfg.gae_lambda, net->cfg.scale,
                             0.f, 0.f, net->ro_tgt, net->ro_adv)))
        return gfail(net, rc, h->err);
    GNET_HIP(net, hipGetLastError());
    return GRL_OK;
}

int grl_gnet_set_greedy(grl_gnet *net, int32_t on) {
    if (!net) return GRL_E_INVALID;
    net->greedy = on ? 1 : 0;
    return GRL_OK;
}

int grl_gnet_eval(grl_gnet *net, int32_t max_steps, int32_t trace_steps) {
    if (!net) return GRL_E_INVALID;
    if (max_steps < 1 || trace_steps < 0) return gfail(net, GRL_E_INVALID, "grl_gnet_eval: max_steps >= 1, trace_steps >= 0");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    if (!h->tk.table) return gfail(net, GRL_E_STATE, "Ticker handle has no price table yet: call grl_ticker_set_table first");
    if (h->cfg.max_episode_steps < 1)
        return gfail(net, GRL_E_STATE, "grl_gnet_eval: the handle has no max_episode_steps, an episode could run past its 1024-row price window");
    if (trace_steps > max_steps) trace_steps = max_steps;
    int rc = ensure_eval_trace(net, trace_steps);
    if (rc) return rc;
    hipStream_t st = h->stream;
    const int E = h->E;
    GEvalArgs v{};
    v.a = gargs(net, E, h->tk.obs, net->win);
    v.win = net->win; v.max_steps = max_steps; v.trace_steps = trace_steps;
    v.total = net->ev_total; v.length = net->ev_len; v.finished = net->ev_fin;
    v.tr_states = net->ev_states; v.tr_probs = net->ev_probs; v.tr_mu = net->ev_mu; v.tr_choices = net->ev_choices;
    v.tr_act = net->ev_actions; v.tr_rew = net->ev_rew; v.tr_done = net->ev_done;
    hipLaunchKernelGGL(gated_eval_kernel, dim3((E + 63) / 64), dim3(256), GATED_LDS, st, v, ticker_params(h));
    GNET_HIP(net, hipGetLastError());
    net->ev_trace = trace_steps;
    net->ev_played = -1;
    net->win_init = 0;      // the windows were the evaluation's: the next rollout starts every env's anew
    // the handle's full reset, as grl_reset(h, NULL, 0) enqueues it
    if ((rc = launch_iota(h, h->done_list, E))) return gfail(net, rc, h->err);
    net->ev_reset_count = E;
    GNET_HIP(net, hipMemcpyAsync(h->done_count, &net->ev_reset_count, 4, hipMemcpyHostToDevice, st));
    if ((rc = ticker_launch_reset(h, h->done_list, h->done_count, E))) return gfail(net, rc, h->err);
    return GRL_OK;
}

int grl_gnet_read_eval(grl_gnet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return gfail(net, GRL_E_INVALID, "grl_gnet_read_eval: bad argument");
    if (net->ev_played == -2) return gfail(net, GRL_E_STATE, "grl_gnet_read_eval: no evaluation yet");
    hipSetDevice(net->h->cfg.device_id);
    GNET_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t E = net->h->E;
    if (net->ev_played < 0) {      // steps the call played = the longest episode
        std::vector<int32_t> len(E);
        GNET_HIP(net, hipMemcpy(len.data(), net->ev_len, E * 4, hipMemcpyDeviceToHost));
        int32_t mx = 0;
        for (int32_t l : len) mx = l > mx ? l : mx;
        net->ev_played = mx;
    }
    const size_t SE = (size_t)(net->ev_trace < net->ev_played ? net->ev_trace : net->ev_played) * E;
    struct { const char *name; const void *p; size_t n; } tab[] = {
        {"total_reward", net->ev_total, E * 8}, {"length", net->ev_len, E * 4}, {"finished", net->ev_fin, E},
        {"states", net->ev_states, SE * GS0 * 4}, {"probs", net->ev_probs, SE * 24}, {"mu", net->ev_mu, SE * 24},
        {"choices", net->ev_choices, SE * 8}, {"actions", net->ev_actions, SE * 16}, {"rewards", net->ev_rew, SE * 4},
        {"dones", net->ev_done, SE * 4}};
    for (auto &e : tab)
        if (!strcmp(which, e.name)) {
            if (bytes != e.n) return gfail(net, GRL_E_SIZE, std::string("grl_gnet_read_eval: wrong size for ") + which);
            if (bytes) GNET_HIP(net, hipMemcpy(host, e.p, bytes, hipMemcpyDeviceToHost));
            return GRL_OK;
        }
    return gfail(net, GRL_E_INVALID, std::string("grl_gnet_read_eval: unknown buffer ") + which);
}

int grl_gnet_train_rollout(grl_gnet *net, float lr0, float *stats_host) {
    if (!net) return GRL_E_INVALID;
    if (!net->T) return gfail(net, GRL_E_STATE, "grl_gnet_train_rollout: no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    const int E = net->h->E, n = net->T * E;
    return train_device(net, n, net->ro_states, net->ro_win, net->ro_choices, net->ro_raw, net->ro_adv, net->ro_tgt, net->ro_wt,
                        1.0f / (float)E, lr0, 1, stats_host);
}

int grl_gnet_read_rollout(grl_gnet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return gfail(net, GRL_E_INVALID, "grl_gnet_read_rollout: bad argument");
    if (!net->T) return gfail(net, GRL_E_STATE, "grl_gnet_read_rollout: no rollout yet");
    const size_t TE = (size_t)net->T * net->h->E, R = net->cfg.rnn_length;
    const void *src = nullptr;
    size_t cnt = 0;
    struct { const char *name; const void *p; size_t n; } tab[] = {
        {"states", net->ro_states, TE * GS0}, {"windows", net->ro_win, TE * R * GD}, {"choices", net->ro_choices, TE * 2},
        {"raw", net->ro_raw, TE * 2}, {"probs", net->ro_probs, TE * 6}, {"mu", net->ro_mu, TE * 6}, {"sigma", net->ro_sigma, TE * 6},
        {"values", net->ro_val, TE}, {"rewards", net->ro_rew, TE}, {"dones", net->ro_done, TE}, {"weights", net->ro_wt, TE},
        {"adv", net->ro_adv, TE}, {"targets", net->ro_tgt, TE}, {"actions", net->ro_act, TE * 4}, {"boot", net->ro_boot, (size_t)net->h->E}};
    for (auto &e : tab)
        if (!strcmp(which, e.name)) { src = e.p; cnt = e.n; }
    if (!src) return gfail(net, GRL_E_INVALID, std::string("grl_gnet_read_rollout: unknown buffer ") + which);
    if (bytes != cnt * 4) return gfail(net, GRL_E_SIZE, std::string("grl_gnet_read_rollout: wrong size for ") + which);
    hipSetDevice(net->h->cfg.device_id);
    GNET_HIP(net, hipStreamSynchronize(net->h->stream));
    GNET_HIP(net, hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // extern "C"
