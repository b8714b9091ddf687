// The A3C Gaussian agent on gfx950 (reference fed_gym/agents/a3c/estimators.py:18-28,241-417 and the worker loop of
// fed_gym/agents/a3c/worker.py:69-341,394-442): a GRU trunk shared by a Gaussian policy (mu and sigma towers) and a value head,
// the device-resident rollout on a Solow or TradeAR1 handle and the A3C update in batched form (include/goldsrl_gaussnet.h).
//
// 148 547 (Solow) / 149 285 (TradeAR1, 2 assets) parameters.  Built like the gated trader (net_gated.hip): a workgroup of 4 waves
// owns 64 samples, activations live in LDS as [feature][sample] rows of LS = 65 floats, every dense layer is an exact-fp32
// v_mfma_f32_32x32x2_f32 GEMM (net_mfma_gemm.inc), the towers run one after another through the same two buffers (256 + 128 rows),
// the update kernels are the gated net's (net_a3c_update.inc).  The kernels are compiled for the two size sets (D = S0 = 2, A = 1 and D = S0 = 5, A = 2).
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

constexpr int LS = 65;        // LDS row stride
constexpr int AH = 32;        // rnn hidden
constexpr int ADMAX = 5;      // largest processed observation (TradeAR1 with 2 assets); Solow: 2
constexpr int AX = 96;        // trunk output: [dense_temporal 64, dense_static 32]
constexpr int AW1 = 256, AW2 = 128;   // static_hidden_size * 2, static_hidden_size
constexpr int AMAXA = 2;      // actions
constexpr int AMAXR = 20;
enum : uint32_t { RS_GAUSS_ACTION = 19 };   // next to RS_GATED_ACTION = 18 (net_gated.hip)

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

#include "net_mfma_gemm.inc"

struct AOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, m1w, m1b, m2w, m2b, m3w, m3b, g1w, g1b, g2w, g2b, g3w, g3b, v1w, v1b, v2w, v2b, total;
};

static AOff gauss_offsets(int D, int A) {
    AOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((D + AH) * 2 * AH); o.gb = take(2 * AH); o.cw = take((D + AH) * AH); o.cb = take(AH);
    o.tw = take(AH * 2 * AH); o.tb = take(2 * AH); o.s1w = take(D * 2 * AH); o.s1b = take(2 * AH); o.s2w = take(2 * AH * AH); o.s2b = take(AH);
    o.m1w = take(AX * AW1); o.m1b = take(AW1); o.m2w = take(AW1 * AW2); o.m2b = take(AW2); o.m3w = take(AW2 * A); o.m3b = take(A);
    o.g1w = take(AX * AW1); o.g1b = take(AW1); o.g2w = take(AW1 * AW2); o.g2b = take(AW2); o.g3w = take(AW2 * A); o.g3b = take(A);
    o.v1w = take(AX * AW1); o.v1b = take(AW1); o.v2w = take(AW1); o.v2b = take(1);
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

// mm_dx of net_mfma_gemm.inc written over the layer's own output X = act(z): X[i][s] = dx * act'(z), ReLU (X > 0) or tanh
// (1 - X^2).  Every element is read and written by the same lane of the same tile, and the GEMM reads only W and dZ, so the dz of
// the layer takes no rows of its own.
template <int ACT>
__device__ __forceinline__ void mm_dx_act_inplace(const float *__restrict__ W, int K, int N, const float *dZ, float *X, int wave, int lane) {
    const int ntiles = ((K + 31) >> 5) * 2, lr = lane & 31, kh = lane >> 5;
#pragma unroll 1
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
            if (i < K) {
                const float x = X[i * LS + s];
                X[i * LS + s] = ACT == FACT_RELU ? (x > 0.f ? acc[r] : 0.f) : acc[r] * (1.0f - x * x);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- LDS layout (rows of LS floats)
constexpr int AL_X = 0;                  // trunk output x (96)
constexpr int AL_DX = AL_X + AX;         // backward: dL/dx of the loss at hand (96)
constexpr int AL_H1 = AL_DX + AX;        // tower layer 1 (256)
constexpr int AL_H2 = AL_H1 + AW1;       // tower layer 2 (128)
constexpr int AL_O = AL_H2 + AW2;        // head outputs / their dz (rows 0..A), backward: mu and its dz (rows 8..8+A)
constexpr int GAUSS_LDS_ROWS = AL_O + 16;
constexpr size_t GAUSS_LDS = (size_t)GAUSS_LDS_ROWS * LS * sizeof(float);       // 154 KB: one workgroup per CU
constexpr int AL_HEAD = AL_DX;           // forward only (it has no dL/dx): mu (A), sigma (A)
// trunk phase, inside the tower rows (free until the towers run)
constexpr int AL_HX = AL_H1;                 // [x_t (D), h or r*h (32)]
constexpr int AL_HS = AL_HX + ADMAX + AH;    // GRU state (32)
constexpr int AL_G = AL_HS + AH;             // gates r, u (64)
constexpr int AL_C = AL_G + 2 * AH;          // candidate (32)
constexpr int AL_ST = AL_C + AH;             // static input (D)
constexpr int AL_S1 = AL_ST + 8;             // dense_static 1 (64)
static_assert(ADMAX <= 8 && AL_S1 + 2 * AH <= AL_O, "trunk rows overflow the tower rows");
// trunk backward, inside the tower rows
constexpr int AB_A = AL_H1, AB_B = AB_A + 64, AB_T = AB_B + 64, AB_DH = AB_T + 64, AB_KEEP = AB_DH + AH;
static_assert(ADMAX + AH <= 64 && AB_KEEP + AH <= AL_O, "trunk backward rows overflow the tower rows");

// per-workgroup scratch of the recomputed forward: per GRU step {h_prev, r, u, c} (128 rows), then h_last (32), dense_static 1
// (64), then the parked mu tower (256 + 128)
__host__ __device__ inline int gauss_scratch_trunk_rows(int R) { return R * 4 * AH + AH + 2 * AH; }
__host__ __device__ inline int gauss_scratch_rows(int R) { return gauss_scratch_trunk_rows(R) + AW1 + AW2; }

// number of window rows with a non-zero entry (true_length, a3c/estimators.py:11-15)
__device__ __forceinline__ int gauss_length(const float *w, int R, int D) {
    int len = 0;
    for (int t = 0; t < R; ++t) {
        float m = 0.f;
        for (int i = 0; i < D; ++i) m = fmaxf(m, fabsf(w[t * D + i]));
        len += m > 0.f ? 1 : 0;
    }
    return len;
}

// threadIdx.x and the wave index.  LOOP (the backward, whose body runs once per 64-sample group): the thread index sits behind a
// compiler barrier, so the address arithmetic each call derives from it stays inside the call instead of being hoisted out of the
// loop over groups and spilled, and the wave index is made uniform again with readfirstlane.  The forward takes both plainly: the
// compiler then knows the wave index to be below 4 and unrolls the tile loops of the GEMMs.
template <bool LOOP = true>
__device__ __forceinline__ int gauss_tid() {
    int t = threadIdx.x;
    if (LOOP) asm volatile("" : "+v"(t));
    return t;
}
template <bool LOOP = true>
__device__ __forceinline__ int gauss_wave(int tid) { return LOOP ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6; }

// rnn_graph_lstm for the group at sbase: x -> X rows.  scr != null: the GRU's per-step activations, h_last and dense_static 1 are
// kept in the workgroup's scratch for the backward.
template <int D, bool LOOP>
__device__ __forceinline__ void gauss_trunk(const AArgs &a, float *lds, int sbase, float *scr) {
    float *X = lds + AL_X * LS, *HX = lds + AL_HX * LS, *HS = lds + AL_HS * LS, *G = lds + AL_G * LS, *Cc = lds + AL_C * LS,
          *ST = lds + AL_ST * LS, *S1 = lds + AL_S1 * LS;
    const int tid = gauss_tid<LOOP>(), lane = tid & 63, wave = gauss_wave<LOOP>(tid);
    const int s = sbase + lane, ss = s < a.n ? s : a.n - 1, R = a.R;      // lanes past n read their own group's last sample
    const float *P = a.P, *w = a.win + (size_t)ss * R * D;
    const int len = gauss_length(w, R, D);
    for (int i = wave; i < AH; i += 4) HS[i * LS + lane] = 0.f;
    for (int i = wave; i < D; i += 4) ST[i * LS + lane] = a.states[(size_t)ss * D + i];
    for (int t = 0; t < R; ++t) {
        // GRUCell (TF 1.4): r,u = sigmoid([x,h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u*h + (1-u)*c
        __syncthreads();
        for (int i = wave; i < D; i += 4) HX[i * LS + lane] = w[t * D + i];
        for (int i = wave; i < AH; i += 4) {
            const float hv = HS[i * LS + lane];
            HX[(D + i) * LS + lane] = hv;
            if (scr) scr[(t * 4 * AH + i) * 64 + lane] = hv;
        }
        __syncthreads();
        mm_fwd<D + AH>(P + a.o.gw, 2 * AH, P + a.o.gb, HX, D + AH, 2 * AH, G, FACT_SIGMOID, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < AH; i += 4) HX[(D + i) * LS + lane] = G[i * LS + lane] * HS[i * LS + lane];
        __syncthreads();
        mm_fwd<D + AH>(P + a.o.cw, AH, P + a.o.cb, HX, D + AH, AH, Cc, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < AH; i += 4) {
            const float u = G[(AH + i) * LS + lane], c = Cc[i * LS + lane];
            if (scr) {
                scr[(t * 4 * AH + AH + i) * 64 + lane] = G[i * LS + lane];
                scr[(t * 4 * AH + 2 * AH + i) * 64 + lane] = u;
                scr[(t * 4 * AH + 3 * AH + i) * 64 + lane] = c;
            }
            if (t < len) HS[i * LS + lane] = u * HS[i * LS + lane] + (1.0f - u) * c;   // dynamic_rnn(sequence_length)
        }
    }
    __syncthreads();
    if (scr)
        for (int i = wave; i < AH; i += 4) scr[(R * 4 * AH + i) * 64 + lane] = HS[i * LS + lane];
    mm_fwd(P + a.o.tw, 2 * AH, P + a.o.tb, HS, AH, 2 * AH, X, FACT_RELU, nullptr, 0, 0, wave, lane);
    mm_fwd(P + a.o.s1w, 2 * AH, P + a.o.s1b, ST, D, 2 * AH, S1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    if (scr)
        for (int i = wave; i < 2 * AH; i += 4) scr[(R * 4 * AH + AH + i) * 64 + lane] = S1[i * LS + lane];
    mm_fwd(P + a.o.s2w, AH, P + a.o.s2b, S1, 2 * AH, AH, X + 2 * AH * LS, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// tower 0 = mu, 1 = sigma: x -> 256 ReLU -> 128 tanh -> A (pre-activation, O rows); tower 2 = value: x -> 256 tanh -> 1
template <int D, bool LOOP>
__device__ __forceinline__ void gauss_tower_fwd(const AArgs &a, float *lds, int tower) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    float *X = lds + AL_X * LS, *H1 = lds + AL_H1 * LS, *H2 = lds + AL_H2 * LS, *O = lds + AL_O * LS;
    const int tid = gauss_tid<LOOP>(), lane = tid & 63, wave = gauss_wave<LOOP>(tid);
    const float *P = a.P;
    if (tower == 2) {
        mm_fwd(P + a.o.v1w, AW1, P + a.o.v1b, X, AX, AW1, H1, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, H1, AW1, 1, O, FACT_NONE, nullptr, 0, 0, wave, lane);
        __syncthreads();
        return;
    }
    const long w1 = tower ? a.o.g1w : a.o.m1w, b1 = tower ? a.o.g1b : a.o.m1b, w2 = tower ? a.o.g2w : a.o.m2w,
               b2 = tower ? a.o.g2b : a.o.m2b, w3 = tower ? a.o.g3w : a.o.m3w, b3 = tower ? a.o.g3b : a.o.m3b;
    mm_fwd(P + w1, AW1, P + b1, X, AX, AW1, H1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w2, AW2, P + b2, H1, AW1, AW2, H2, FACT_TANH, nullptr, 0, 0, wave, lane);
    __syncthreads();
    mm_fwd(P + w3, A, P + b3, H2, AW2, A, O, FACT_NONE, nullptr, 0, 0, wave, lane);
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
    float *O = lds + AL_O * LS, *MU = lds + AL_HEAD * LS, *SG = MU + AMAXA * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane;
    const bool valid = s < a.n;
    bool on = valid;
    if (a.gate) {      // every wave sees the same 64 samples: the exit is uniform over the workgroup
        on = valid && a.gate[s] != 0.f;
        if (__ballot(on) == 0ull) return;
    }
    gauss_trunk<D, false>(a, lds, sbase, nullptr);
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

// trunk backward for one loss: DX rows hold dL/dx; weight gradients go to G (a slab half)
template <int D>
__device__ __forceinline__ void gauss_trunk_bwd(const AArgs &a, float *lds, int sbase, const float *scr, float *G, int len) {
    float *X = lds + AL_X * LS, *DX = lds + AL_DX * LS, *BA = lds + AB_A * LS, *BB = lds + AB_B * LS, *BT = lds + AB_T * LS,
          *DH = lds + AB_DH * LS, *KEEP = lds + AB_KEEP * LS;
    const int tid = gauss_tid(), lane = tid & 63, wave = gauss_wave(tid), s = sbase + lane, ss = s < a.n ? s : 0, R = a.R;
    const float *P = a.P, *w = a.win + (size_t)ss * R * D;
    auto S = [&](int f) { return scr[f * 64 + lane]; };
    __syncthreads();
    // static path: x[64..96) = relu(S1 W2 + b2), S1 = relu(states W1 + b1)
    for (int i = wave; i < AH; i += 4) BB[i * LS + lane] = X[(2 * AH + i) * LS + lane] > 0.f ? DX[(2 * AH + i) * LS + lane] : 0.f;
    for (int i = wave; i < 2 * AH; i += 4) BA[i * LS + lane] = S(R * 4 * AH + AH + i);
    __syncthreads();
    mm_wgrad(BA, BB, 2 * AH, AH, G + a.o.s2w, G + a.o.s2b, wave, lane);
    mm_dx(P + a.o.s2w, 2 * AH, AH, BB, BT, false, wave, lane);
    __syncthreads();
    for (int i = wave; i < 2 * AH; i += 4) BB[i * LS + lane] = BA[i * LS + lane] > 0.f ? BT[i * LS + lane] : 0.f;
    __syncthreads();
    for (int i = wave; i < D; i += 4) BA[i * LS + lane] = a.states[(size_t)ss * D + i];
    __syncthreads();
    mm_wgrad(BA, BB, D, 2 * AH, G + a.o.s1w, G + a.o.s1b, wave, lane);
    __syncthreads();
    // dense_temporal
    for (int i = wave; i < 2 * AH; i += 4) BB[i * LS + lane] = X[i * LS + lane] > 0.f ? DX[i * LS + lane] : 0.f;
    for (int i = wave; i < AH; i += 4) BA[i * LS + lane] = S(R * 4 * AH + i);
    __syncthreads();
    mm_wgrad(BA, BB, AH, 2 * AH, G + a.o.tw, G + a.o.tb, wave, lane);
    mm_dx(P + a.o.tw, AH, 2 * AH, BB, DH, false, wave, lane);
    // GRU, back through time with the sequence-length mask
    for (int t = R - 1; t >= 0; --t) {
        const bool act = t < len;
        __syncthreads();
        for (int i = wave; i < D; i += 4) BA[i * LS + lane] = w[t * D + i];
        for (int i = wave; i < AH; i += 4) {
            const int f = t * 4 * AH;
            const float hp = S(f + i), r = S(f + AH + i), u = S(f + 2 * AH + i), c = S(f + 3 * AH + i);
            const float dhn = act ? DH[i * LS + lane] : 0.f;
            KEEP[i * LS + lane] = dhn * u;
            BB[i * LS + lane] = dhn * (1.0f - u) * (1.0f - c * c);             // dz of the candidate
            BB[(AH + i) * LS + lane] = dhn * (hp - c) * u * (1.0f - u);         // dz of the update gate (kept for later)
            BA[(D + i) * LS + lane] = r * hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, D + AH, AH, G + a.o.cw, G + a.o.cb, wave, lane);
        mm_dx(P + a.o.cw, D + AH, AH, BB, BT, false, wave, lane);
        __syncthreads();
        for (int i = wave; i < AH; i += 4) {
            const int f = t * 4 * AH;
            const float hp = S(f + i), r = S(f + AH + i);
            const float drh = BT[(D + i) * LS + lane];
            KEEP[i * LS + lane] += drh * r;
            BB[i * LS + lane] = drh * hp * r * (1.0f - r);                     // dz of the reset gate
            BA[(D + i) * LS + lane] = hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, D + AH, 2 * AH, G + a.o.gw, G + a.o.gb, wave, lane);
        mm_dx(P + a.o.gw, D + AH, 2 * AH, BB, BT, false, wave, lane);
        __syncthreads();
        if (act)
            for (int i = wave; i < AH; i += 4) DH[i * LS + lane] = KEEP[i * LS + lane] + BT[(D + i) * LS + lane];
    }
    __syncthreads();
}

// back through a 96 -> 256 ReLU -> 128 tanh -> A tower whose dz of the last layer is in the O rows; d x (=|+=) into DX
template <int D>
__device__ __forceinline__ void gauss_tower_bwd(const AArgs &a, float *lds, float *G, long w1, long b1, long w2, long b2, long w3, long b3, bool accumulate) {
    constexpr int A = D == 2 ? 1 : 2;      // Solow: 1 action, TradeAR1 with 2 assets: 2
    float *X = lds + AL_X * LS, *DX = lds + AL_DX * LS, *H1 = lds + AL_H1 * LS, *H2 = lds + AL_H2 * LS, *O = lds + AL_O * LS;
    const int tid = gauss_tid(), lane = tid & 63, wave = gauss_wave(tid);
    const float *P = a.P;
    __syncthreads();
    mm_wgrad(H2, O, AW2, A, G + w3, G + b3, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_TANH>(P + w3, AW2, A, O, H2, wave, lane);
    __syncthreads();
    mm_wgrad(H1, H2, AW1, AW2, G + w2, G + b2, wave, lane);
    __syncthreads();
    mm_dx_act_inplace<FACT_RELU>(P + w2, AW1, AW2, H2, H1, wave, lane);
    __syncthreads();
    mm_wgrad(X, H1, AX, AW1, G + w1, G + b1, wave, lane);
    mm_dx(P + w1, AX, AW1, H1, DX, accumulate, wave, lane);
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
    float *O = lds + AL_O * LS, *H1 = lds + AL_H1 * LS, *MUZ = O + 8 * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long Pn = a.o.total;
    float *Gp = a.slab + (size_t)blockIdx.x * 2 * Pn, *Gv = Gp + Pn;
    float *scr = a.scratch + (size_t)blockIdx.x * gauss_scratch_rows(a.R) * 64;
    float *park = scr + (size_t)gauss_scratch_trunk_rows(a.R) * 64;
    const int groups = (a.n + 63) / 64;
    double lp = 0.0, lv = 0.0, ent = 0.0, wsum = 0.0;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int sbase = grp * 64, s = sbase + lane;
        const bool valid = s < a.n;
        const int ss = valid ? s : 0;
        const float wt = valid ? (a.wt ? a.wt[ss] : 1.0f) : 0.f;
        const float c = a.mult * wt, adv = a.adv[ss], cp = c * adv;
        const int len = gauss_length(a.win + (size_t)ss * a.R * D, a.R, D);
        gauss_trunk<D, true>(a, lds, sbase, scr);
        // ---- mu tower forward; its hidden layers (H1 and H2 are adjacent rows) wait in the scratch while the sigma tower runs
        gauss_tower_fwd<D, true>(a, lds, 0);
        if (wave < A) MUZ[wave * LS + lane] = O[wave * LS + lane];
        for (int i = wave; i < AW1 + AW2; i += 4) park[i * 64 + lane] = H1[i * LS + lane];
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
        for (int i = wave; i < AW1 + AW2; i += 4) H1[i * LS + lane] = park[i * 64 + lane];
        if (wave < A) O[wave * LS + lane] = MUZ[wave * LS + lane];
        gauss_tower_bwd<D>(a, lds, Gp, a.o.m1w, a.o.m1b, a.o.m2w, a.o.m2b, a.o.m3w, a.o.m3b, true);
        gauss_trunk_bwd<D>(a, lds, sbase, scr, Gp, len);
        // ---- value head
        gauss_tower_fwd<D, true>(a, lds, 2);
        if (wave == 0) {
            const float v = a.scale * O[lane], tg = a.tgt[ss], dv = v - tg;
            O[lane] = c * dv;                               // d/dz of c * 0.5 (scale z - t)^2 / scale
            if (valid) lv += (double)(c * 0.5f * dv * dv / a.scale);
        }
        __syncthreads();
        mm_wgrad(H1, O, AW1, 1, Gv + a.o.v2w, Gv + a.o.v2b, wave, lane);
        __syncthreads();
        for (int i = wave; i < AW1; i += 4) {
            const float h = H1[i * LS + lane];
            H1[i * LS + lane] = a.P[a.o.v2w + i] * O[lane] * (1.0f - h * h);
        }
        __syncthreads();
        mm_wgrad(lds + AL_X * LS, H1, AX, AW1, Gv + a.o.v1w, Gv + a.o.v1b, wave, lane);
        mm_dx(a.P + a.o.v1w, AX, AW1, H1, lds + AL_DX * LS, false, wave, lane);
        gauss_trunk_bwd<D>(a, lds, sbase, scr, Gv, len);
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

#include "net_a3c_update.inc"

// ---------------------------------------------------------------------------------------------- rollout
// window of env e: rows [0, min(k+1, R)) hold the episode's last processed states (current last), zero rows after; k = kstep[e]
__device__ __forceinline__ void gauss_window_restart(float *win, int R, int D, const float *obs) {
    for (int i = 0; i < D; ++i) win[i] = obs[i];
    for (int i = D; i < R * D; ++i) win[i] = 0.f;
}

// the window after one more step whose processed state is o; k = the new step index in the episode
__device__ __forceinline__ void gauss_window_push(float *w, int R, int D, int k, const float *o) {
    if (k < R) {
        for (int i = 0; i < D; ++i) w[k * D + i] = o[i];
    } else {
        for (int i = 0; i < (R - 1) * D; ++i) w[i] = w[i + D];
        for (int i = 0; i < D; ++i) w[(R - 1) * D + i] = o[i];
    }
}

// the window rule behind an env step (k = the env's step in its episode before it, o = the observation after it): a new row,
// or a restart at the reset observation where the episode ended.  Returns the new k.
__device__ __forceinline__ int gauss_window_step(float *w, int R, int D, int k, bool done, const float *o) {
    if (done) {
        gauss_window_restart(w, R, D, o);
        return 0;
    }
    gauss_window_push(w, R, D, k + 1, o);
    return k + 1;
}

// before a rollout: envs the handle (re)set since (elapsed 0), or all of them the first time, start a new window
__global__ void gauss_sync_kernel(const int32_t *__restrict__ elapsed, const float *__restrict__ obs, float *__restrict__ win,
                                  int32_t *__restrict__ kstep, int E, int R, int D, int all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (all || elapsed[e] == 0) {
        gauss_window_restart(win + (size_t)e * R * D, R, D, obs + (size_t)e * D);
        kstep[e] = 0;
    }
}

// record the step's inputs: states[t], windows[t], weights[t] (the worker records a transition once its history has R rows)
__global__ void gauss_record_kernel(const float *__restrict__ obs, const float *__restrict__ win, const int32_t *__restrict__ kstep, int E,
                                    int R, int D, float *__restrict__ st, float *__restrict__ wn, float *__restrict__ wt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    for (int i = 0; i < D; ++i) st[(size_t)e * D + i] = obs[(size_t)e * D + i];
    for (int i = 0; i < R * D; ++i) wn[(size_t)e * R * D + i] = win[(size_t)e * R * D + i];
    if (wt) wt[e] = kstep[e] >= R - 1 ? 1.0f : 0.0f;
}

// after the env step: reward, done, mask; the window restarts on done (the observation is the reset one) or takes the new row.
// term_obs != null (always_bootstrap): where the episode ended, the terminal observation and the window that ends in it are kept
// for the terminal value pass (worker.py:252-257) before the window restarts.
__global__ void gauss_post_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done, const float *__restrict__ obs,
                                  const float *__restrict__ term_obs, float *__restrict__ win, int32_t *__restrict__ kstep, int E, int R, int D,
                                  float *__restrict__ rew, float *__restrict__ dn, float *__restrict__ mask, float *__restrict__ term_st,
                                  float *__restrict__ term_wn) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool d = done[e] != 0;
    rew[e] = reward[e];
    dn[e] = d ? 1.0f : 0.0f;
    mask[e] = d ? 0.0f : 1.0f;
    float *w = win + (size_t)e * R * D;
    const float *o = obs + (size_t)e * D;
    const int k = kstep[e];
    if (d && term_obs) {
        const float *to = term_obs + (size_t)e * D;
        gauss_window_push(w, R, D, k + 1, to);
        for (int i = 0; i < D; ++i) term_st[(size_t)e * D + i] = to[i];
        for (int i = 0; i < R * D; ++i) term_wn[(size_t)e * R * D + i] = w[i];
    }
    kstep[e] = gauss_window_step(w, R, D, k, d, o);
}

// The worker's GAE (worker.py:241-294) per env column, cut at episode ends: delta_t = r_t + g V_next - V_t with V_next = V_{t+1}, or
// behind a finished episode term[t] (always_bootstrap) / done_penalty = 0; A_t = delta_t + g lam m_t A_{t+1}; target = A_t + V_t,
// adv = A_t / scale.  float64 running sums like returns_column (rollout_dev.h).  boot[e] becomes the value behind the last step.
__global__ void gauss_returns_kernel(const float *__restrict__ r, const float *__restrict__ v, const float *__restrict__ dn,
                                     const float *__restrict__ term, float *__restrict__ boot, int T, int E, float gamma, float lam, float scale,
                                     int always_bootstrap, float *__restrict__ y, float *__restrict__ adv) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double g = (double)gamma, gl = g * (double)lam;
    double run = 0.0, vnext = (double)boot[e];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * E + e;
        const bool d = dn[i] != 0.f;
        if (d) vnext = always_bootstrap ? (double)term[i] : 0.0;
        if (d && t == T - 1) boot[e] = (float)vnext;
        const double vt = (double)v[i];
        const double delta = (double)r[i] + g * vnext - vt;
        run = delta + (d ? 0.0 : gl * run);
        y[i] = (float)(run + vt);
        adv[i] = (float)(run / (double)scale);
        vnext = vt;
    }
}

#include "net_gauss_eval.inc"

}  // namespace grl

struct grl_anet {
    grl_handle *h;
    grl_anet_config cfg;
    std::string err;
    grl::AOff off;
    int D, A;                                     // processed observation = temporal row width, actions
    float *params, *grads, *msp, *msv, *stats;    // grads: [policy P | value P]
    double *stats64;                              // 4 loss sums, then 2 x kA3cSumsqBlocks partial sums
    int64_t global_step;
    uint64_t act_counter;
    int greedy;                                   // grl_anet_set_greedy
    // host-sample staging
    float *d_states, *d_win, *d_raw, *d_adv, *d_tgt, *d_wt, *d_mu, *d_sigma, *d_vals;
    // training workspace (grown on demand)
    float *slab, *scratch;
    int ws_blocks;
    // rollout
    float *win;                                   // (E,R,D) each env's current window
    int32_t *kstep;
    int win_init;
    int T;
    float *ro_states, *ro_win, *ro_raw, *ro_mu, *ro_sigma, *ro_val, *ro_rew, *ro_done, *ro_mask, *ro_wt, *ro_adv, *ro_tgt;
    float *ro_act;                                // (T,E,A) the action each env was stepped with
    float *ro_term_st, *ro_term_wn, *ro_term_val; // ro_term_st / ro_term_wn: always_bootstrap only
    float *ro_boot, *boot_states, *boot_win, *term_obs;
    // grl_anet_eval: per-env results, the step's actions, the trace of the first ev_trace steps
    double *ev_total;
    int32_t *ev_len;
    uint8_t *ev_fin;
    float *ev_act, *ev_states, *ev_mu, *ev_actions, *ev_rew, *ev_done;
    int32_t ev_reset_count;                       // E, the source of the reset list's count (outlives the async copy)
    int ev_trace, ev_trace_cap, ev_played;        // ev_played: -1 until grl_anet_read_eval has looked, -2 before any evaluation
    std::vector<void *> allocs, ro_allocs, ws_allocs, ev_allocs;
};

namespace grl {

static int afail(grl_anet *n, int code, const std::string &msg) {
    if (n) n->err = msg;
    return code;
}
#define ANET_HIP(n, call)                                                                                  \
    do {                                                                                                   \
        hipError_t _e = (call);                                                                            \
        if (_e != hipSuccess) return afail(n, GRL_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
static int aalloc(grl_anet *n, T **p, size_t count, std::vector<void *> &list) {
    ANET_HIP(n, hipMalloc((void **)p, (count ? count : 1) * sizeof(T)));
    list.push_back(*p);
    ANET_HIP(n, hipMemsetAsync(*p, 0, (count ? count : 1) * sizeof(T), n->h->stream));
    return GRL_OK;
}

static const float *anet_obs(const grl_anet *net) { return net->h->cfg.env_kind == GRL_ENV_SOLOW ? net->h->so.obs : net->h->tr.obs; }

static AArgs aargs(grl_anet *net, int n, const float *states, const float *win) {
    AArgs a{};
    a.P = net->params; a.o = net->off; a.n = n; a.R = net->cfg.rnn_length; a.scale = net->cfg.scale;
    a.states = states; a.win = win; a.mult = 1.0f;
    return a;
}

static int launch_fwd(grl_anet *net, const AArgs &a) {
    if (net->D == 2) hipLaunchKernelGGL(gauss_forward_kernel<2>, dim3((a.n + 63) / 64), dim3(256), GAUSS_LDS, net->h->stream, a);
    else hipLaunchKernelGGL(gauss_forward_kernel<5>, dim3((a.n + 63) / 64), dim3(256), GAUSS_LDS, net->h->stream, a);
    ANET_HIP(net, hipGetLastError());
    return GRL_OK;
}

// the backward's slabs and scratch for `blocks` workgroups
static int ensure_ws(grl_anet *net, int blocks) {
    if (blocks <= net->ws_blocks) return GRL_OK;
    ANET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ws_allocs) hipFree(p);
    net->ws_allocs.clear();
    net->ws_blocks = 0;
    int rc = aalloc(net, &net->slab, (size_t)blocks * 2 * net->off.total, net->ws_allocs);
    if (!rc) rc = aalloc(net, &net->scratch, (size_t)blocks * gauss_scratch_rows(net->cfg.rnn_length) * 64, net->ws_allocs);
    if (!rc) net->ws_blocks = blocks;
    return rc;
}

// gradients of both losses over n device-resident samples, then norms, clip factors and (apply) both RMSProp steps
static int train_device(grl_anet *net, int n, const float *states, const float *win, const float *raw, const float *adv, const float *tgt,
                        const float *wt, float mult, float lr0, int apply, float *stats_host) {
    hipStream_t st = net->h->stream;
    const int groups = (n + 63) / 64, blocks = groups < 256 ? groups : 256;      // 154 KB of LDS: one workgroup per CU
    int rc = ensure_ws(net, blocks);
    if (rc) return rc;
    const long P = net->off.total;
    ANET_HIP(net, hipMemsetAsync(net->slab, 0, (size_t)blocks * 2 * P * sizeof(float), st));
    ANET_HIP(net, hipMemsetAsync(net->stats64, 0, 4 * sizeof(double), st));
    AArgs a = aargs(net, n, states, win);
    a.raw = raw; a.adv = adv; a.tgt = tgt; a.wt = wt; a.mult = mult;
    a.slab = net->slab; a.scratch = net->scratch; a.stats64 = net->stats64;
    if (net->D == 2) hipLaunchKernelGGL(gauss_backward_kernel<2>, dim3(blocks), dim3(256), GAUSS_LDS, st, a);
    else hipLaunchKernelGGL(gauss_backward_kernel<5>, dim3(blocks), dim3(256), GAUSS_LDS, st, a);
    hipLaunchKernelGGL(flat_slab_reduce_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(1024), 0, st, net->slab, blocks, 2 * P, net->grads);
    hipLaunchKernelGGL(a3c_sumsq_kernel, dim3(kA3cSumsqBlocks, 2), dim3(256), 0, st, net->grads, P, net->stats64 + 4);
    // tf.train.exponential_decay(lr0, global_step, decay_steps, rate, staircase=False), global_step before the update
    const float lr = (float)((double)lr0 * pow((double)net->cfg.lr_decay_rate, (double)net->global_step / (double)net->cfg.lr_decay_steps));
    hipLaunchKernelGGL(a3c_finalize_kernel, dim3(1), dim3(64), 0, st, net->stats64, net->stats64 + 4, (double)net->A, net->cfg.clip_norm, lr,
                       net->stats);
    if (apply) {
        hipLaunchKernelGGL(a3c_rmsprop_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, net->params, net->grads, net->msp, net->msv, P,
                           net->off.m1w, net->off.v1w, net->stats, net->cfg.rms_decay, net->cfg.rms_epsilon);
        net->global_step += 2;      // both train ops increment it (estimators.py:325-328, 409-412)
    }
    ANET_HIP(net, hipGetLastError());
    ANET_HIP(net, hipStreamSynchronize(st));
    if (stats_host) {
        float s[6];
        ANET_HIP(net, hipMemcpy(s, net->stats, sizeof(s), hipMemcpyDeviceToHost));
        for (int i = 0; i < 6; ++i) stats_host[i] = s[i];
    }
    return GRL_OK;
}

static int ensure_rollout(grl_anet *net, int T) {
    if (T == net->T) return GRL_OK;
    ANET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ro_allocs) hipFree(p);
    net->ro_allocs.clear();
    net->T = 0;
    const size_t E = net->h->E, R = net->cfg.rnn_length, TE = (size_t)T * E, D = net->D, A = net->A;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = aalloc(net, p, cnt, net->ro_allocs); };
    Al(&net->ro_states, TE * D); Al(&net->ro_win, TE * R * D); Al(&net->ro_raw, TE * A); Al(&net->ro_mu, TE * A); Al(&net->ro_sigma, TE * A);
    Al(&net->ro_val, TE); Al(&net->ro_rew, TE); Al(&net->ro_done, TE); Al(&net->ro_mask, TE); Al(&net->ro_wt, TE); Al(&net->ro_adv, TE);
    Al(&net->ro_tgt, TE); Al(&net->ro_act, TE * A); Al(&net->ro_term_val, TE);
    net->ro_term_st = net->ro_term_wn = nullptr;
    if (net->cfg.always_bootstrap) { Al(&net->ro_term_st, TE * D); Al(&net->ro_term_wn, TE * R * D); }
    if (rc == GRL_OK) net->T = T;
    return rc;
}

// the trace buffers of grl_anet_eval for `steps` steps (they only grow)
static int ensure_eval_trace(grl_anet *net, int steps) {
    if (steps <= net->ev_trace_cap) return GRL_OK;
    ANET_HIP(net, hipStreamSynchronize(net->h->stream));
    for (void *p : net->ev_allocs) hipFree(p);
    net->ev_allocs.clear();
    net->ev_trace_cap = -1;
    const size_t SE = (size_t)steps * net->h->E, D = net->D, A = net->A;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = aalloc(net, p, cnt, net->ev_allocs); };
    Al(&net->ev_states, SE * D); Al(&net->ev_mu, SE * A); Al(&net->ev_actions, SE * A); Al(&net->ev_rew, SE); Al(&net->ev_done, SE);
    if (rc == GRL_OK) net->ev_trace_cap = steps;
    return rc;
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
    if (!h || !cfg || !out) return GRL_E_INVALID;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(grl_anet_config)) return fail(h, GRL_E_INVALID, "grl_anet_create: config size mismatch");
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW, trade = h->cfg.env_kind == GRL_ENV_TRADE && h->cfg.n_assets == 2;
    if (!solow && !trade) return fail(h, GRL_E_INVALID, "grl_anet_create: the Gaussian agent needs a Solow handle or a TradeAR1 handle with 2 assets");
    if (cfg->rnn_length < 1 || cfg->rnn_length > AMAXR || cfg->max_samples < 1 || cfg->lr_decay_steps < 1 || !(cfg->scale != 0.f) ||
        !(cfg->gae_lambda > 0.f && cfg->gae_lambda <= 1.f))
        return fail(h, GRL_E_INVALID, "grl_anet_create: config out of range (rnn_length 1..20)");
    if (cfg->always_bootstrap != (solow ? 1 : 0))
        return fail(h, GRL_E_INVALID, solow ? "grl_anet_create: a Solow handle needs always_bootstrap = 1" :
                                              "grl_anet_create: a TradeAR1 handle needs always_bootstrap = 0");
    hipSetDevice(h->cfg.device_id);
    grl_anet *n = new grl_anet();
    n->h = h; n->cfg = *cfg;
    n->D = solow ? 2 : 5; n->A = solow ? 1 : 2;
    n->off = gauss_offsets(n->D, n->A);
    n->global_step = 0; n->act_counter = 0; n->greedy = 0; n->ws_blocks = 0; n->win_init = 0; n->T = 0;
    n->ev_trace = 0; n->ev_trace_cap = -1; n->ev_played = -2;
    const size_t ms = cfg->max_samples, P = n->off.total, R = cfg->rnn_length, E = h->E, D = n->D, A = n->A;
    int rc = GRL_OK;
    auto Al = [&](float **p, size_t cnt) { if (rc == GRL_OK) rc = aalloc(n, p, cnt, n->allocs); };
    Al(&n->params, P); Al(&n->grads, 2 * P); Al(&n->msp, P); Al(&n->msv, P); Al(&n->stats, 8);
    Al(&n->d_states, ms * D); Al(&n->d_win, ms * R * D); Al(&n->d_raw, ms * A); Al(&n->d_adv, ms); Al(&n->d_tgt, ms); Al(&n->d_wt, ms);
    Al(&n->d_mu, ms * A); Al(&n->d_sigma, ms * A); Al(&n->d_vals, ms);
    Al(&n->win, E * R * D); Al(&n->ro_boot, E); Al(&n->boot_states, E * D); Al(&n->boot_win, E * R * D);
    Al(&n->term_obs, E * D); Al(&n->ev_act, E * A);
    if (rc == GRL_OK) rc = aalloc(n, &n->kstep, E, n->allocs);
    if (rc == GRL_OK) rc = aalloc(n, &n->ev_total, E, n->allocs);
    if (rc == GRL_OK) rc = aalloc(n, &n->ev_len, E, n->allocs);
    if (rc == GRL_OK) rc = aalloc(n, &n->ev_fin, E, n->allocs);
    if (rc == GRL_OK) rc = aalloc(n, &n->stats64, 4 + 2 * kA3cSumsqBlocks, n->allocs);
    if (rc == GRL_OK) {      // RMSProp ms starts at ones (TF 1.x)
        hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, n->msp, (long)P, 1.0f);
        hipLaunchKernelGGL(a3c_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, n->msv, (long)P, 1.0f);
        hipError_t e = hipGetLastError();
        const void *kernels[3] = {solow ? (const void *)gauss_forward_kernel<2> : (const void *)gauss_forward_kernel<5>,
                                  solow ? (const void *)gauss_backward_kernel<2> : (const void *)gauss_backward_kernel<5>,
                                  solow ? (const void *)gauss_eval_kernel<2, SolowParams> : (const void *)gauss_eval_kernel<5, TradeParams>};
        for (const void *k : kernels)
            if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GAUSS_LDS);
        if (e != hipSuccess) rc = afail(n, GRL_E_HIP, std::string("grl_anet_create: ") + hipGetErrorString(e));
    }
    if (rc != GRL_OK) {
        fail(h, rc, "grl_anet_create: " + n->err);
        grl_anet_destroy(n);
        return rc;
    }
    hipStreamSynchronize(h->stream);
    *out = n;
    return GRL_OK;
}

int grl_anet_destroy(grl_anet *n) {
    if (!n) return GRL_OK;
    grl_sync_for_destroy(n->h);
    for (void *p : n->allocs) hipFree(p);
    for (void *p : n->ro_allocs) hipFree(p);
    for (void *p : n->ws_allocs) hipFree(p);
    for (void *p : n->ev_allocs) hipFree(p);
    delete n;
    return GRL_OK;
}

const char *grl_anet_last_error(const grl_anet *n) { return n ? n->err.c_str() : "null net"; }
int64_t grl_anet_num_params(const grl_anet *n) { return n ? n->off.total : 0; }

static int acopy(grl_anet *n, float *dev, float *host, int64_t cnt, int64_t want, bool to_dev) {
    if (!n || !host) return afail(n, GRL_E_INVALID, "null argument");
    if (cnt != want) return afail(n, GRL_E_SIZE, "length must be num_params");
    hipSetDevice(n->h->cfg.device_id);
    ANET_HIP(n, hipStreamSynchronize(n->h->stream));
    ANET_HIP(n, hipMemcpy(to_dev ? (void *)dev : (void *)host, to_dev ? (const void *)host : (const void *)dev, (size_t)cnt * 4,
                          to_dev ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_anet_set_params(grl_anet *n, const float *host, int64_t cnt) { return acopy(n, n ? n->params : nullptr, (float *)host, cnt, n ? n->off.total : 0, true); }
int grl_anet_get_params(grl_anet *n, float *host, int64_t cnt) { return acopy(n, n ? n->params : nullptr, host, cnt, n ? n->off.total : 0, false); }
int grl_anet_get_grads(grl_anet *n, int32_t which, float *host, int64_t cnt) {
    if (n && which != GRL_ANET_POLICY && which != GRL_ANET_VALUE) return afail(n, GRL_E_INVALID, "grl_anet_get_grads: which is 0 or 1");
    return acopy(n, n ? n->grads + (which ? n->off.total : 0) : nullptr, host, cnt, n ? n->off.total : 0, false);
}

int grl_anet_get_optimizer_state(grl_anet *n, float *msp, float *msv, int64_t cnt, int64_t *step) {
    int rc = acopy(n, n ? n->msp : nullptr, msp, cnt, n ? n->off.total : 0, false);
    if (!rc) rc = acopy(n, n->msv, msv, cnt, n->off.total, false);
    if (!rc && step) *step = n->global_step;
    return rc;
}

int grl_anet_set_optimizer_state(grl_anet *n, const float *msp, const float *msv, int64_t cnt, int64_t step) {
    if (n && step < 0) return afail(n, GRL_E_INVALID, "global step must be >= 0");
    int rc = acopy(n, n ? n->msp : nullptr, (float *)msp, cnt, n ? n->off.total : 0, true);
    if (!rc) rc = acopy(n, n->msv, (float *)msv, cnt, n->off.total, true);
    if (!rc) n->global_step = step;
    return rc;
}

int grl_anet_get_action_counter(grl_anet *n, uint64_t *out) {
    if (!n || !out) return GRL_E_INVALID;
    *out = n->act_counter;
    return GRL_OK;
}

int grl_anet_set_action_counter(grl_anet *n, uint64_t v) {
    if (!n) return GRL_E_INVALID;
    n->act_counter = v;
    return GRL_OK;
}

int grl_anet_predict(grl_anet *net, int32_t n, const float *states, const float *windows, float *mu, float *sigma, float *values) {
    if (!net || n <= 0 || !states || !windows) return afail(net, GRL_E_INVALID, "grl_anet_predict: bad argument");
    if (n > net->cfg.max_samples) return afail(net, GRL_E_SIZE, "grl_anet_predict: n exceeds max_samples");
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    const size_t R = net->cfg.rnn_length, D = net->D, A = net->A;
    ANET_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * D * 4, hipMemcpyHostToDevice, st));
    ANET_HIP(net, hipMemcpyAsync(net->d_win, windows, (size_t)n * R * D * 4, hipMemcpyHostToDevice, st));
    AArgs a = aargs(net, n, net->d_states, net->d_win);
    a.mu = net->d_mu; a.sigma = net->d_sigma; a.vals = net->d_vals;
    int rc = launch_fwd(net, a);
    if (rc) return rc;
    ANET_HIP(net, hipStreamSynchronize(st));
    if (mu) ANET_HIP(net, hipMemcpy(mu, net->d_mu, (size_t)n * A * 4, hipMemcpyDeviceToHost));
    if (sigma) ANET_HIP(net, hipMemcpy(sigma, net->d_sigma, (size_t)n * A * 4, hipMemcpyDeviceToHost));
    if (values) ANET_HIP(net, hipMemcpy(values, net->d_vals, (size_t)n * 4, hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_anet_train(grl_anet *net, int32_t n, const float *states, const float *windows, const float *raw, const float *adv,
                   const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host) {
    if (!net || n <= 0 || !states || !windows || !raw || !adv || !targets) return afail(net, GRL_E_INVALID, "grl_anet_train: bad argument");
    if (n > net->cfg.max_samples) return afail(net, GRL_E_SIZE, "grl_anet_train: n exceeds max_samples");
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    const size_t R = net->cfg.rnn_length, D = net->D, A = net->A;
    ANET_HIP(net, hipMemcpyAsync(net->d_states, states, (size_t)n * D * 4, hipMemcpyHostToDevice, st));
    ANET_HIP(net, hipMemcpyAsync(net->d_win, windows, (size_t)n * R * D * 4, hipMemcpyHostToDevice, st));
    ANET_HIP(net, hipMemcpyAsync(net->d_raw, raw, (size_t)n * A * 4, hipMemcpyHostToDevice, st));
    ANET_HIP(net, hipMemcpyAsync(net->d_adv, adv, (size_t)n * 4, hipMemcpyHostToDevice, st));
    ANET_HIP(net, hipMemcpyAsync(net->d_tgt, targets, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (weights) ANET_HIP(net, hipMemcpyAsync(net->d_wt, weights, (size_t)n * 4, hipMemcpyHostToDevice, st));
    return train_device(net, n, net->d_states, net->d_win, net->d_raw, net->d_adv, net->d_tgt, weights ? net->d_wt : nullptr, grad_mult, lr0,
                        apply_update, stats_host);
}

int grl_anet_rollout(grl_anet *net, int32_t T) {
    if (!net || T < 1) return afail(net, GRL_E_INVALID, "grl_anet_rollout: T >= 1");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    int rc = ensure_rollout(net, T);
    if (rc) return rc;
    hipStream_t st = h->stream;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E, R = net->cfg.rnn_length, D = net->D, A = net->A, eb = (E + 255) / 256, ab = net->cfg.always_bootstrap;
    const float *obs = anet_obs(net);
    const size_t TE = (size_t)T * E;
    if (ab) ANET_HIP(net, hipMemsetAsync(net->ro_term_val, 0, TE * 4, st));      // steps that end no episode read 0
    hipLaunchKernelGGL(gauss_sync_kernel, dim3(eb), dim3(256), 0, st, h->elapsed, obs, net->win, net->kstep, E, R, D, net->win_init ? 0 : 1);
    net->win_init = 1;
    for (int t = 0; t < T; ++t) {
        const size_t o = (size_t)t * E;
        hipLaunchKernelGGL(gauss_record_kernel, dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, D, net->ro_states + o * D,
                           net->ro_win + o * R * D, net->ro_wt + o);
        AArgs a = aargs(net, E, net->ro_states + o * D, net->ro_win + o * R * D);
        a.mu = net->ro_mu + o * A; a.sigma = net->ro_sigma + o * A; a.vals = net->ro_val + o;
        a.act = net->ro_act + o * A; a.raw_out = net->ro_raw + o * A; a.tanh_action = solow ? 0 : 1;
        a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset; a.counter = (uint32_t)(net->act_counter + (uint64_t)t);
        a.greedy = net->greedy;
        if ((rc = launch_fwd(net, a))) return rc;
        rc = solow ? solow_launch_step(h, net->ro_act + o * A, ab ? net->term_obs : nullptr) : trade_launch_step(h, net->ro_act + o * A);
        if (rc) return afail(net, rc, h->err);
        if ((rc = episodes_launch_account(h))) return afail(net, rc, h->err);
        hipLaunchKernelGGL(gauss_post_kernel, dim3(eb), dim3(256), 0, st, h->reward, h->done, obs, ab ? net->term_obs : (const float *)nullptr,
                           net->win, net->kstep, E, R, D, net->ro_rew + o, net->ro_done + o, net->ro_mask + o, ab ? net->ro_term_st + o * D : (float *)nullptr,
                           ab ? net->ro_term_wn + o * R * D : (float *)nullptr);
    }
    if (!net->greedy) net->act_counter += (uint64_t)T;      // a greedy rollout draws nothing
    // bootstrap: V of the window after the last step; with always_bootstrap also V behind every finished episode (workgroups whose
    // 64 samples ended none leave at once); then the worker's GAE (worker.py:241-294)
    hipLaunchKernelGGL(gauss_record_kernel, dim3(eb), dim3(256), 0, st, obs, net->win, net->kstep, E, R, D, net->boot_states, net->boot_win,
                       (float *)nullptr);
    AArgs b = aargs(net, E, net->boot_states, net->boot_win);
    b.vals = net->ro_boot;
    if ((rc = launch_fwd(net, b))) return rc;
    if (ab) {
        AArgs c = aargs(net, (int)TE, net->ro_term_st, net->ro_term_wn);
        c.gate = net->ro_done; c.vals = net->ro_term_val;
        if ((rc = launch_fwd(net, c))) return rc;
    }
    hipLaunchKernelGGL(gauss_returns_kernel, dim3(eb), dim3(256), 0, st, net->ro_rew, net->ro_val, net->ro_done, net->ro_term_val, net->ro_boot, T, E,
                       net->cfg.gamma, net->cfg.gae_lambda, net->cfg.scale, ab, net->ro_tgt, net->ro_adv);
    ANET_HIP(net, hipGetLastError());
    return GRL_OK;
}

int grl_anet_set_greedy(grl_anet *net, int32_t on) {
    if (!net) return GRL_E_INVALID;
    net->greedy = on ? 1 : 0;
    return GRL_OK;
}

int grl_anet_eval(grl_anet *net, int32_t max_steps, int32_t trace_steps) {
    if (!net) return GRL_E_INVALID;
    if (max_steps < 1 || trace_steps < 0) return afail(net, GRL_E_INVALID, "grl_anet_eval: max_steps >= 1, trace_steps >= 0");
    grl_handle *h = net->h;
    hipSetDevice(h->cfg.device_id);
    if (trace_steps > max_steps) trace_steps = max_steps;
    int rc = ensure_eval_trace(net, trace_steps);
    if (rc) return rc;
    hipStream_t st = h->stream;
    const bool solow = h->cfg.env_kind == GRL_ENV_SOLOW;
    const int E = h->E;
    AEvalArgs v{};
    v.a = aargs(net, E, anet_obs(net), net->win);
    v.win = net->win; v.act = net->ev_act; v.tanh_action = solow ? 0 : 1; v.max_steps = max_steps; v.trace_steps = trace_steps;
    v.total = net->ev_total; v.length = net->ev_len; v.finished = net->ev_fin;
    v.tr_states = net->ev_states; v.tr_mu = net->ev_mu; v.tr_act = net->ev_actions; v.tr_rew = net->ev_rew; v.tr_done = net->ev_done;
    if (solow) {
        SolowParams S = solow_params(h);
        hipLaunchKernelGGL((gauss_eval_kernel<2, SolowParams>), dim3((E + 63) / 64), dim3(256), GAUSS_LDS, st, v, S);
    } else {
        TradeParams S = trade_params(h);
        hipLaunchKernelGGL((gauss_eval_kernel<5, TradeParams>), dim3((E + 63) / 64), dim3(256), GAUSS_LDS, st, v, S);
    }
    ANET_HIP(net, hipGetLastError());
    net->ev_trace = trace_steps;
    net->ev_played = -1;
    net->win_init = 0;      // the windows were the evaluation's: the next rollout starts every env's anew
    // the handle's full reset (for Solow with the tape draw), as grl_reset(h, NULL, 0) enqueues it
    if ((rc = launch_iota(h, h->done_list, E))) return afail(net, rc, h->err);
    net->ev_reset_count = E;
    ANET_HIP(net, hipMemcpyAsync(h->done_count, &net->ev_reset_count, 4, hipMemcpyHostToDevice, st));
    rc = solow ? solow_launch_reset(h, h->done_list, h->done_count, E, true) : trade_launch_reset(h, h->done_list, h->done_count, E);
    if (rc) return afail(net, rc, h->err);
    return GRL_OK;
}

int grl_anet_read_eval(grl_anet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return afail(net, GRL_E_INVALID, "grl_anet_read_eval: bad argument");
    if (net->ev_played == -2) return afail(net, GRL_E_STATE, "grl_anet_read_eval: no evaluation yet");
    hipSetDevice(net->h->cfg.device_id);
    ANET_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t E = net->h->E, D = net->D, A = net->A;
    if (net->ev_played < 0) {      // steps the call played = the longest episode
        std::vector<int32_t> len(E);
        ANET_HIP(net, hipMemcpy(len.data(), net->ev_len, E * 4, hipMemcpyDeviceToHost));
        int32_t mx = 0;
        for (int32_t l : len) mx = l > mx ? l : mx;
        net->ev_played = mx;
    }
    const size_t SE = (size_t)(net->ev_trace < net->ev_played ? net->ev_trace : net->ev_played) * E;
    struct { const char *name; const void *p; size_t n; } tab[] = {
        {"total_reward", net->ev_total, E * 8}, {"length", net->ev_len, E * 4}, {"finished", net->ev_fin, E},
        {"states", net->ev_states, SE * D * 4}, {"mu", net->ev_mu, SE * A * 4}, {"actions", net->ev_actions, SE * A * 4},
        {"rewards", net->ev_rew, SE * 4}, {"dones", net->ev_done, SE * 4}};
    for (auto &e : tab)
        if (!strcmp(which, e.name)) {
            if (bytes != e.n) return afail(net, GRL_E_SIZE, std::string("grl_anet_read_eval: wrong size for ") + which);
            if (bytes) ANET_HIP(net, hipMemcpy(host, e.p, bytes, hipMemcpyDeviceToHost));
            return GRL_OK;
        }
    return afail(net, GRL_E_INVALID, std::string("grl_anet_read_eval: unknown buffer ") + which);
}

int grl_anet_train_rollout(grl_anet *net, float lr0, float *stats_host) {
    if (!net) return GRL_E_INVALID;
    if (!net->T) return afail(net, GRL_E_STATE, "grl_anet_train_rollout: no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    const int E = net->h->E, n = net->T * E;
    return train_device(net, n, net->ro_states, net->ro_win, net->ro_raw, net->ro_adv, net->ro_tgt, net->ro_wt, 1.0f / (float)E, lr0, 1,
                        stats_host);
}

int grl_anet_read_rollout(grl_anet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return afail(net, GRL_E_INVALID, "grl_anet_read_rollout: bad argument");
    if (!net->T) return afail(net, GRL_E_STATE, "grl_anet_read_rollout: no rollout yet");
    const size_t TE = (size_t)net->T * net->h->E, R = net->cfg.rnn_length, D = net->D, A = net->A;
    const void *src = nullptr;
    size_t cnt = 0;
    struct { const char *name; const void *p; size_t n; } tab[] = {
        {"states", net->ro_states, TE * D}, {"windows", net->ro_win, TE * R * D}, {"raw", net->ro_raw, TE * A}, {"mu", net->ro_mu, TE * A},
        {"sigma", net->ro_sigma, TE * A}, {"actions", net->ro_act, TE * A}, {"values", net->ro_val, TE}, {"rewards", net->ro_rew, TE}, {"dones", net->ro_done, TE},
        {"weights", net->ro_wt, TE}, {"adv", net->ro_adv, TE}, {"targets", net->ro_tgt, TE}, {"term_values", net->ro_term_val, TE},
        {"term_states", net->ro_term_st, TE * D}, {"term_windows", net->ro_term_wn, TE * R * D}, {"boot", net->ro_boot, (size_t)net->h->E}};
    for (auto &e : tab)
        if (!strcmp(which, e.name)) { src = e.p; cnt = e.n; }
    if (!src && cnt) return afail(net, GRL_E_STATE, std::string("grl_anet_read_rollout: ") + which + " exists with always_bootstrap = 1 only");
    if (!src) return afail(net, GRL_E_INVALID, std::string("grl_anet_read_rollout: unknown buffer ") + which);
    if (bytes != cnt * 4) return afail(net, GRL_E_SIZE, std::string("grl_anet_read_rollout: wrong size for ") + which);
    hipSetDevice(net->h->cfg.device_id);
    ANET_HIP(net, hipStreamSynchronize(net->h->stream));
    ANET_HIP(net, hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // extern "C"
