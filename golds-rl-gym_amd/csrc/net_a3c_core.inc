// Included inside namespace grl by net_gated.hip (the Ticker gated trader), net_gauss.hip (the Gaussian Solow / TradeAR1 agent) and
// net_discrete.hip (the discrete savings-grid Solow agent): the device code the A3C nets share -- the LDS row layout, the GRU trunk forward and backward, the in-place dx, the window rules
// with their per-env kernels and the update.  static / inline: every including translation unit has its own copy.  The including
// file defines first
//   A3C_DPAD      rows kept for the temporal row x_t (its widest D; the layout, and with it the compiled code, depends on it)
//   A3C_PAD_LAST  the sample the forward trunk reads for lanes past n: n - 1 (true: their own group's last sample) or 0.  n - 1 is
//                 the rule to prefer; the gated net stays at 0 because its greedy rollout measured 0.4 us per step slower with
//                 n - 1 (LABNOTES K)
// The trunks are duck-typed on the net's argument block: a.P, a.o.gw .. a.o.s2b, a.n, a.R, a.states, a.win.

constexpr int LS = 65;        // LDS row stride
constexpr int NH = 32;        // rnn hidden
constexpr int NX = 96;        // trunk output: [dense_temporal 64, dense_static 32]
constexpr int NW1 = 256, NW2 = 128;   // static_hidden_size * 2, static_hidden_size
constexpr int MAXR = 20;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

#include "net_mfma_gemm.inc"

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
constexpr int L_X = 0;                   // trunk output x (96)
constexpr int L_DX = L_X + NX;           // backward: dL/dx of the loss at hand (96)
constexpr int L_H1 = L_DX + NX;          // tower layer 1 (256)
constexpr int L_H2 = L_H1 + NW1;         // tower layer 2 (128)
constexpr int L_O = L_H2 + NW2;          // head outputs / their dz (16)
constexpr size_t A3C_LDS = (size_t)(L_O + 16) * LS * sizeof(float);      // 154 KB: one workgroup per CU
constexpr int L_HEAD = L_DX;             // forward only (it has no dL/dx): the heads' activated outputs
// trunk phase, inside the tower rows (free until the towers run)
constexpr int L_HX = L_H1;               // [x_t (D), h or r*h (32)]
constexpr int L_HS = L_HX + A3C_DPAD + NH;   // GRU state (32)
constexpr int L_G = L_HS + NH;           // gates r, u (64)
constexpr int L_C = L_G + 2 * NH;        // candidate (32)
constexpr int L_ST = L_C + NH;           // static input (S0)
constexpr int L_S1 = L_ST + 8;           // dense_static 1 (64)
static_assert(A3C_DPAD <= 8 && L_S1 + 2 * NH <= L_O, "trunk rows overflow the tower rows");
// trunk backward, inside the tower rows
constexpr int B_A = L_H1, B_B = B_A + 64, B_T = B_B + 64, B_DH = B_T + 64, B_KEEP = B_DH + NH;
static_assert(A3C_DPAD + NH <= 64 && B_KEEP + NH <= L_O, "trunk backward rows overflow the tower rows");

// per-workgroup scratch of the recomputed forward: per GRU step {h_prev, r, u, c} (128 rows), then h_last (32), dense_static 1 (64)
__host__ __device__ inline int a3c_scratch_trunk_rows(int R) { return R * 4 * NH + NH + 2 * NH; }

// number of window rows with a non-zero entry (true_length, a3c/estimators.py:11-15)
__device__ __forceinline__ int a3c_length(const float *w, int R, int D) {
    int len = 0;
    for (int t = 0; t < R; ++t) {
        float m = 0.f;
        for (int i = 0; i < D; ++i) m = fmaxf(m, fabsf(w[t * D + i]));
        len += m > 0.f ? 1 : 0;
    }
    return len;
}

// threadIdx.x and the wave index.  LOOP (the Gaussian backward, whose body runs once per 64-sample group): the thread index sits
// behind a compiler barrier, so the address arithmetic each call derives from it stays inside the call instead of being hoisted out
// of the loop over groups and spilled, and the wave index is made uniform again with readfirstlane.  Without it both are taken
// plainly: the compiler then knows the wave index to be below 4 and unrolls the tile loops of the GEMMs.
template <bool LOOP = true>
__device__ __forceinline__ int a3c_tid() {
    int t = threadIdx.x;
    if (LOOP) asm volatile("" : "+v"(t));
    return t;
}
template <bool LOOP = true>
__device__ __forceinline__ int a3c_wave(int tid) { return LOOP ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6; }

// rnn_graph_lstm for the group at sbase: x -> X rows.  D = the temporal row's width, S0 = the static input's.  scr != null: the
// GRU's per-step activations, h_last and dense_static 1 are kept in the workgroup's scratch for the backward.
template <int D, int S0, bool LOOP, typename ARGS>
__device__ __forceinline__ void a3c_trunk(const ARGS &a, float *lds, int sbase, float *scr) {
    float *X = lds + L_X * LS, *HX = lds + L_HX * LS, *HS = lds + L_HS * LS, *G = lds + L_G * LS, *Cc = lds + L_C * LS,
          *ST = lds + L_ST * LS, *S1 = lds + L_S1 * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid);
    const int s = sbase + lane, ss = s < a.n ? s : (A3C_PAD_LAST ? a.n - 1 : 0), R = a.R;
    const float *P = a.P, *w = a.win + (size_t)ss * R * D;
    const int len = a3c_length(w, R, D);
    for (int i = wave; i < NH; i += 4) HS[i * LS + lane] = 0.f;
    for (int i = wave; i < S0; i += 4) ST[i * LS + lane] = a.states[(size_t)ss * S0 + i];
    for (int t = 0; t < R; ++t) {
        // GRUCell (TF 1.4): r,u = sigmoid([x,h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u*h + (1-u)*c
        __syncthreads();
        for (int i = wave; i < D; i += 4) HX[i * LS + lane] = w[t * D + i];
        for (int i = wave; i < NH; i += 4) {
            const float hv = HS[i * LS + lane];
            HX[(D + i) * LS + lane] = hv;
            if (scr) scr[(t * 4 * NH + i) * 64 + lane] = hv;
        }
        __syncthreads();
        mm_fwd<D + NH>(P + a.o.gw, 2 * NH, P + a.o.gb, HX, D + NH, 2 * NH, G, FACT_SIGMOID, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < NH; i += 4) HX[(D + i) * LS + lane] = G[i * LS + lane] * HS[i * LS + lane];
        __syncthreads();
        mm_fwd<D + NH>(P + a.o.cw, NH, P + a.o.cb, HX, D + NH, NH, Cc, FACT_TANH, nullptr, 0, 0, wave, lane);
        __syncthreads();
        for (int i = wave; i < NH; i += 4) {
            const float u = G[(NH + i) * LS + lane], c = Cc[i * LS + lane];
            if (scr) {
                scr[(t * 4 * NH + NH + i) * 64 + lane] = G[i * LS + lane];
                scr[(t * 4 * NH + 2 * NH + i) * 64 + lane] = u;
                scr[(t * 4 * NH + 3 * NH + i) * 64 + lane] = c;
            }
            if (t < len) HS[i * LS + lane] = u * HS[i * LS + lane] + (1.0f - u) * c;   // dynamic_rnn(sequence_length)
        }
    }
    __syncthreads();
    if (scr)
        for (int i = wave; i < NH; i += 4) scr[(R * 4 * NH + i) * 64 + lane] = HS[i * LS + lane];
    mm_fwd(P + a.o.tw, 2 * NH, P + a.o.tb, HS, NH, 2 * NH, X, FACT_RELU, nullptr, 0, 0, wave, lane);
    mm_fwd(P + a.o.s1w, 2 * NH, P + a.o.s1b, ST, S0, 2 * NH, S1, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
    if (scr)
        for (int i = wave; i < 2 * NH; i += 4) scr[(R * 4 * NH + NH + i) * 64 + lane] = S1[i * LS + lane];
    mm_fwd(P + a.o.s2w, NH, P + a.o.s2b, S1, 2 * NH, NH, X + 2 * NH * LS, FACT_RELU, nullptr, 0, 0, wave, lane);
    __syncthreads();
}

// trunk backward for one loss: DX rows hold dL/dx; weight gradients go to G (a slab half).  Lanes past n read sample 0 here, for
// both nets: the backward kernels that call this read their own per-sample inputs (weights, advantages, the length) the same way,
// and every dz of such a lane is multiplied by its weight 0, so which real sample it reads changes no result.
template <int D, int S0, bool LOOP, typename ARGS>
__device__ __forceinline__ void a3c_trunk_bwd(const ARGS &a, float *lds, int sbase, const float *scr, float *G, int len) {
    float *X = lds + L_X * LS, *DX = lds + L_DX * LS, *BA = lds + B_A * LS, *BB = lds + B_B * LS, *BT = lds + B_T * LS,
          *DH = lds + B_DH * LS, *KEEP = lds + B_KEEP * LS;
    const int tid = a3c_tid<LOOP>(), lane = tid & 63, wave = a3c_wave<LOOP>(tid), s = sbase + lane, ss = s < a.n ? s : 0, R = a.R;
    const float *P = a.P, *w = a.win + (size_t)ss * R * D;
    auto S = [&](int f) { return scr[f * 64 + lane]; };
    __syncthreads();
    // static path: x[64..96) = relu(S1 W2 + b2), S1 = relu(states W1 + b1)
    for (int i = wave; i < NH; i += 4) BB[i * LS + lane] = X[(2 * NH + i) * LS + lane] > 0.f ? DX[(2 * NH + i) * LS + lane] : 0.f;
    for (int i = wave; i < 2 * NH; i += 4) BA[i * LS + lane] = S(R * 4 * NH + NH + i);
    __syncthreads();
    mm_wgrad(BA, BB, 2 * NH, NH, G + a.o.s2w, G + a.o.s2b, wave, lane);
    mm_dx(P + a.o.s2w, 2 * NH, NH, BB, BT, false, wave, lane);
    __syncthreads();
    for (int i = wave; i < 2 * NH; i += 4) BB[i * LS + lane] = BA[i * LS + lane] > 0.f ? BT[i * LS + lane] : 0.f;
    __syncthreads();
    for (int i = wave; i < S0; i += 4) BA[i * LS + lane] = a.states[(size_t)ss * S0 + i];
    __syncthreads();
    mm_wgrad(BA, BB, S0, 2 * NH, G + a.o.s1w, G + a.o.s1b, wave, lane);
    __syncthreads();
    // dense_temporal
    for (int i = wave; i < 2 * NH; i += 4) BB[i * LS + lane] = X[i * LS + lane] > 0.f ? DX[i * LS + lane] : 0.f;
    for (int i = wave; i < NH; i += 4) BA[i * LS + lane] = S(R * 4 * NH + i);
    __syncthreads();
    mm_wgrad(BA, BB, NH, 2 * NH, G + a.o.tw, G + a.o.tb, wave, lane);
    mm_dx(P + a.o.tw, NH, 2 * NH, BB, DH, false, wave, lane);
    // GRU, back through time with the sequence-length mask
    for (int t = R - 1; t >= 0; --t) {
        const bool act = t < len;
        __syncthreads();
        for (int i = wave; i < D; i += 4) BA[i * LS + lane] = w[t * D + i];
        for (int i = wave; i < NH; i += 4) {
            const int f = t * 4 * NH;
            const float hp = S(f + i), r = S(f + NH + i), u = S(f + 2 * NH + i), c = S(f + 3 * NH + i);
            const float dhn = act ? DH[i * LS + lane] : 0.f;
            KEEP[i * LS + lane] = dhn * u;
            BB[i * LS + lane] = dhn * (1.0f - u) * (1.0f - c * c);             // dz of the candidate
            BB[(NH + i) * LS + lane] = dhn * (hp - c) * u * (1.0f - u);         // dz of the update gate (kept for later)
            BA[(D + i) * LS + lane] = r * hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, D + NH, NH, G + a.o.cw, G + a.o.cb, wave, lane);
        mm_dx(P + a.o.cw, D + NH, NH, BB, BT, false, wave, lane);
        __syncthreads();
        for (int i = wave; i < NH; i += 4) {
            const int f = t * 4 * NH;
            const float hp = S(f + i), r = S(f + NH + i);
            const float drh = BT[(D + i) * LS + lane];
            KEEP[i * LS + lane] += drh * r;
            BB[i * LS + lane] = drh * hp * r * (1.0f - r);                     // dz of the reset gate
            BA[(D + i) * LS + lane] = hp;
        }
        __syncthreads();
        mm_wgrad(BA, BB, D + NH, 2 * NH, G + a.o.gw, G + a.o.gb, wave, lane);
        mm_dx(P + a.o.gw, D + NH, 2 * NH, BB, BT, false, wave, lane);
        __syncthreads();
        if (act)
            for (int i = wave; i < NH; i += 4) DH[i * LS + lane] = KEEP[i * LS + lane] + BT[(D + i) * LS + lane];
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------- update
// sums of squares in float64 of the two gradients [policy P | value P]: kA3cSumsqBlocks partial sums each, added in order by
// a3c_finalize_kernel
constexpr int kA3cSumsqBlocks = 32;
static __global__ __launch_bounds__(256) void a3c_sumsq_kernel(const float *__restrict__ g, long n, double *__restrict__ out) {
    __shared__ double red[256];
    const float *gg = g + (size_t)blockIdx.y * n;
    const long per = (n + kA3cSumsqBlocks - 1) / kA3cSumsqBlocks, lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += (double)gg[i] * (double)gg[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.y * kA3cSumsqBlocks + blockIdx.x] = red[0];
}

// stats: policy loss, value loss, entropy mean, policy norm, value norm, lr; then the two clip factors (tf.clip_by_global_norm)
// heads: entropy terms per sample (stats64[2] sums weight * entropy over them)
static __global__ void a3c_finalize_kernel(const double *__restrict__ stats64, const double *__restrict__ sumsq, double heads, float clip_norm,
                                           float lr, float *__restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sp = 0.0, sv = 0.0;
    for (int b = 0; b < kA3cSumsqBlocks; ++b) { sp += sumsq[b]; sv += sumsq[kA3cSumsqBlocks + b]; }
    const float np_ = (float)sqrt(sp), nv = (float)sqrt(sv);
    stats[0] = (float)stats64[0];
    stats[1] = (float)stats64[1];
    stats[2] = stats64[3] > 0.0 ? (float)(stats64[2] / (heads * stats64[3])) : 0.f;
    stats[3] = np_; stats[4] = nv; stats[5] = lr;
    stats[6] = clip_norm > 0.f ? clip_norm / fmaxf(np_, clip_norm) : 1.0f;
    stats[7] = clip_norm > 0.f ? clip_norm / fmaxf(nv, clip_norm) : 1.0f;
}

// both RMSProp steps (TF 1.x, momentum 0): ms <- rho ms + (1-rho) g^2 ; step = lr g / sqrt(ms + eps).  The policy gradient covers
// [0, v1w), the value gradient [0, c1w) (the trunk) and [v1w, total): the trunk takes both steps, each from the same pre-update parameters.
static __global__ void a3c_rmsprop_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ msp, float *__restrict__ msv, long n,
                                     long c1w, long v1w, const float *__restrict__ stats, float rho, float eps) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float lr = stats[5];
    float w = p[i];
    if (i < v1w) {
        const float gi = g[i] * stats[6];
        const float m = rho * msp[i] + (1.0f - rho) * gi * gi;
        msp[i] = m;
        w = w - lr * gi / sqrtf(m + eps);
    }
    if (i < c1w || i >= v1w) {
        const float gi = g[n + i] * stats[7];
        const float m = rho * msv[i] + (1.0f - rho) * gi * gi;
        msv[i] = m;
        w = w - lr * gi / sqrtf(m + eps);
    }
    p[i] = w;
}

static __global__ void a3c_fill_kernel(float *__restrict__ p, long n, float v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---------------------------------------------------------------------------------------------- rollout
// window of env e: rows [0, min(k+1, R)) hold the episode's last temporal rows (current last), zero rows after; k = kstep[e].
// row = the temporal row (D wide) of an observation: the observation at toff (Ticker: 3, behind the static-only part; else 0).
// D is an int, or a std::integral_constant where a kernel was tuned with the width known inside these functions.
template <typename DT>
__device__ __forceinline__ void a3c_window_restart(float *win, int R, DT D, const float *row) {
    for (int i = 0; i < D; ++i) win[i] = row[i];
    for (int i = D; i < R * D; ++i) win[i] = 0.f;
}

// the window after one more step whose temporal row is given; k = the new step index in the episode
template <typename DT>
__device__ __forceinline__ void a3c_window_push(float *w, int R, DT D, int k, const float *row) {
    if (k < R) {
        for (int i = 0; i < D; ++i) w[k * D + i] = row[i];
    } else {
        for (int i = 0; i < (R - 1) * D; ++i) w[i] = w[i + D];
        for (int i = 0; i < D; ++i) w[(R - 1) * D + i] = row[i];
    }
}

// the window rule behind an env step (k = the env's step in its episode before it, row = of the observation after it): a new row,
// or a restart at the reset observation where the episode ended.  Returns the new k.
template <typename DT>
__device__ __forceinline__ int a3c_window_step(float *w, int R, DT D, int k, bool done, const float *row) {
    if (done) {
        a3c_window_restart(w, R, D, row);
        return 0;
    }
    k += 1;
    a3c_window_push(w, R, D, k, row);
    return k;
}

// The per-env kernels of a rollout.  S0, D, toff (the observation's width, the temporal row's width and its offset in the observation)
// are ints, or std::integral_constants where a net's widths are fixed: the gated trader's copies then unroll as they did as kernels
// of its own (with run-time widths its rollout step took 2.5 us longer, LABNOTES K).
//
// before a rollout: envs the handle (re)set since (elapsed 0), or all of them the first time, start a new window
template <typename ST, typename DT, typename TT>
static __global__ void a3c_sync_kernel(const int32_t *__restrict__ elapsed, const float *__restrict__ obs, float *__restrict__ win,
                                       int32_t *__restrict__ kstep, int E, int R, ST S0, DT D, TT toff, int all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (all || elapsed[e] == 0) {
        a3c_window_restart(win + (size_t)e * R * D, R, D, obs + (size_t)e * S0 + toff);
        kstep[e] = 0;
    }
}

// record the step's inputs: states[t], windows[t], weights[t] (the worker records a transition once its history has R rows)
template <typename ST, typename DT>
static __global__ void a3c_record_kernel(const float *__restrict__ obs, const float *__restrict__ win, const int32_t *__restrict__ kstep, int E,
                                         int R, ST S0, DT D, float *__restrict__ st, float *__restrict__ wn, float *__restrict__ wt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    for (int i = 0; i < S0; ++i) st[(size_t)e * S0 + i] = obs[(size_t)e * S0 + i];
    for (int i = 0; i < R * D; ++i) wn[(size_t)e * R * D + i] = win[(size_t)e * R * D + i];
    if (wt) wt[e] = kstep[e] >= R - 1 ? 1.0f : 0.0f;
}

// after the env step: reward, done, mask; the window restarts on done (the observation is the reset one) or takes the new row.
// term_obs != null (the Gaussian net's always_bootstrap): where the episode ended, the terminal observation and the window that
// ends in it are kept for the terminal value pass (worker.py:252-257) before the window restarts.
template <typename ST, typename DT, typename TT>
static __global__ void a3c_post_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done, const float *__restrict__ obs,
                                       const float *__restrict__ term_obs, float *__restrict__ win, int32_t *__restrict__ kstep, int E, int R, ST S0,
                                       DT D, TT toff, float *__restrict__ rew, float *__restrict__ dn, float *__restrict__ mask,
                                       float *__restrict__ term_st, float *__restrict__ term_wn) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool d = done[e] != 0;
    rew[e] = reward[e];
    dn[e] = d ? 1.0f : 0.0f;
    mask[e] = d ? 0.0f : 1.0f;
    float *w = win + (size_t)e * R * D;
    const int k = kstep[e];
    if (d && term_obs) {
        const float *to = term_obs + (size_t)e * S0;
        a3c_window_push(w, R, D, k + 1, to + toff);
        for (int i = 0; i < S0; ++i) term_st[(size_t)e * S0 + i] = to[i];
        for (int i = 0; i < R * D; ++i) term_wn[(size_t)e * R * D + i] = w[i];
    }
    kstep[e] = a3c_window_step(w, R, D, k, d, obs + (size_t)e * S0 + toff);
}

// The worker's GAE (worker.py:241-294) per env column, cut at episode ends: delta_t = r_t + g V_next - V_t with V_next = V_{t+1}, or
// behind a finished episode term[t] (always_bootstrap) / done_penalty = 0; A_t = delta_t + g lam m_t A_{t+1}; target = A_t + V_t,
// adv = A_t / scale.  float64 running sums like returns_column (rollout_dev.h).  boot[e] becomes the value behind the last step.
// A template so that only the nets that launch it (the Gaussian and the discrete agent) carry it.
template <typename F>
static __global__ void a3c_returns_kernel(const F *__restrict__ r, const F *__restrict__ v, const F *__restrict__ dn,
                                          const F *__restrict__ term, F *__restrict__ boot, int T, int E, float gamma, float lam, float scale,
                                          int always_bootstrap, F *__restrict__ y, F *__restrict__ adv) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double g = (double)gamma, gl = g * (double)lam;
    double run = 0.0, vnext = (double)boot[e];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * E + e;
        const bool d = dn[i] != 0.f;
        if (d) vnext = always_bootstrap ? (double)term[i] : 0.0;
        if (d && t == T - 1) boot[e] = (F)vnext;
        const double vt = (double)v[i];
        const double delta = (double)r[i] + g * vnext - vt;
        run = delta + (d ? 0.0 : gl * run);
        y[i] = (F)(run + vt);
        adv[i] = (F)(run / (double)scale);
        vnext = vt;
    }
}
