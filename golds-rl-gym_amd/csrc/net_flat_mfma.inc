// Included by net_flat.hip (inside namespace grl): FlatPolicyVNetwork forward / backward kernels.
//
// One workgroup = 4 waves = one group of 64 samples.  Activations live in LDS as [feature][sample] rows of LS = 65
// floats.  Every dense layer (GRU gates and candidate, the MLPs, the heads) is a small GEMM against the group's 64
// samples and runs on v_mfma_f32_32x32x2_f32 (exact fp32): 32 x 32 tiles of (output feature, sample), (input
// feature, sample) or (input feature, output feature), distributed over the four waves -- operands come straight from
// the [feature][sample] rows (a lane reads row (lane & 31), column k + (lane >> 5): conflict free with stride 65) and
// from the row-major weight matrices in global memory (31 k parameters: cache resident).
//   forward:          Y[o][s]  = b[o] + sum_i W[i][o] X[i][s]          A = W^T (global), B = X (LDS)
//   data gradient:    dX[i][s] = sum_o W[i][o] dZ[o][s]                A = W (global),   B = dZ (LDS)
//   weight gradient:  dW[i][o] += sum_s X[i][s] dZ[o][s]               A = X (LDS),      B = dZ^T (LDS), 32 MFMAs per tile
// Elementwise work (activations, GRU state update, masks, loss terms) is spread over all 256 threads.
// The previous version of these kernels kept one wave per workgroup with scalar-weight FMA loops and 64-long LDS dot
// products per weight: 1 wave per CU, 2 LDS reads per MAC in the weight gradient -- 20-100x slower.

#include "net_mfma_gemm.inc"

// LDS rows (LS floats each).  Buffers of the GRU phase alias buffers that are first written after it, so a workgroup needs
// 304 rows = 79 KB and two workgroups share a CU.
constexpr int FL_X96 = 0;                // [dense_temporal (64), dense_static (32)]  (written after the GRU phase)
constexpr int FL_HX = FL_X96;            // GRU phase: [x_t (D <= 33), h / r*h (32)], 65 rows
constexpr int FL_H = FL_X96 + 96;        // current GRU state: 32
constexpr int FL_T1 = FL_H + 32;         // 64
constexpr int FL_G = FL_T1;              // GRU phase: gates r (32), u (32)
constexpr int FL_T2 = FL_T1 + 64;        // 32
constexpr int FL_C = FL_T2;              // GRU phase: candidate, 32
constexpr int FL_ST = FL_T2 + 32;        // static input: 64 (read once, right after the GRU phase)
constexpr int FL_SM = FL_ST + 64;        // head pre-activations: 16
constexpr int FLAT_FWD_ROWS = FL_SM + 16;

// sample-private scalars of the thread's sample (every wave holds a copy): rows of the history that exist, true_length
__device__ __forceinline__ void flat_lengths(const FlatArgs &a, int ss, bool valid, const float *&hrow, int &hstep, int &nrows, int &len) {
    const bool synth = a.nhist != nullptr;
    hrow = synth ? a.states + (long)ss * a.S0 : a.hist + (long)ss * a.T * a.D;
    hstep = synth ? 0 : a.D;      // synthesized window: every valid row is the current state
    nrows = a.T;
    if (synth) { int nh = a.nhist[ss]; nh = nh < 1 ? 1 : nh; nrows = nh < a.T ? nh : a.T; }
    len = 0;      // true_length (a3c/estimators.py:11-15): number of rows with a non-zero entry
    if (synth) {      // every existing row IS the current state: one pass over its D values instead of T x D loads
        float m = 0.f;
        for (int i = 0; i < a.D; ++i) m = fmaxf(m, fabsf(hrow[i]));
        len = (valid && m > 0.f) ? nrows : 0;
        return;
    }
    for (int t = 0; t < a.T; ++t) {
        float m = 0.f;
        for (int i = 0; i < a.D; ++i) m = fmaxf(m, fabsf(t < nrows ? hrow[t * hstep + i] : 0.f));
        len += (valid && m > 0.f) ? 1 : 0;
    }
}

// the third source beside "dense" and "synthesized": the true window as a strided view of the rollout's state slab (net_flat_window.inc).
// a.nhist[ss] rows, a.wstride * S0 floats apart, the last one a.states[ss] itself; true_length over the rows as for a dense window
__device__ __forceinline__ void flat_lengths_win(const FlatArgs &a, int ss, bool valid, const float *&hrow, int &hstep, int &nrows, int &len) {
    int nh = a.nhist[ss];
    nh = nh < 1 ? 1 : nh;
    nrows = nh < a.T ? nh : a.T;
    hrow = a.states + ((long)ss - (long)(nrows - 1) * a.wstride) * a.S0;
    hstep = a.wstride * a.S0;
    len = 0;
    for (int t = 0; t < nrows; ++t) {
        float m = 0.f;
        for (int i = 0; i < a.D; ++i) m = fmaxf(m, fabsf(hrow[(long)t * hstep + i]));
        len += (valid && m > 0.f) ? 1 : 0;
    }
}

// WLDS: the GRU's two kernels ([x,h] -> gates 64, candidate 32: (D+32) x 96 floats, 25 KB at D = 33) are copied to LDS behind the
// activation rows once per workgroup; the 2 x T MFMA loops of the recurrence then read them with ds_read instead of one
// global load per MFMA.  The forward is latency bound (SQ counters at 8 192 TradeAR1 envs: 59 % of the wave cycles parked at
// s_waitcnt / barriers, matrix pipe busy 10 %), and a grid of <= 256 workgroups (one per CU) leaves LDS to spare.
//
// flat_forward_core is the forward pass of ONE group of 64 samples; two callers share it so that they compute the same bits:
//   flat_forward_kernel            one launch per forward pass: inputs from global memory (a.states / a.hist / a.nhist)
//   flat_rollout_kernel            the persistent T-step actor loop (net_flat_rollout.inc): `staged` -- the static-input rows ST
//                                  already hold the group's current observation in LDS, the window is the PAAC worker's
//                                  (nrows copies of it, quirk Q11), and the heads are left in the LDS rows MUL / SGL / VSL
struct FwdLocal {
    bool staged;            // ST rows, nrows and len come from the caller
    int nrows, len;
    float *MUL, *SGL, *VSL; // LDS rows [A][LS], [A][LS], [LS] or nullptr
    bool weights_ready;     // WLDS: the GRU kernels are already in LDS (copied once per rollout, not once per forward)
    float *ws;              // staged only: the training workspace this forward fills, or nullptr
    int sample0;            // staged only: the workspace sample of the group's first member (t * E + sbase in a rollout)
    long long *ts;          // stage timestamps of workgroup 0 (tools/flat_stage_times.py), or nullptr
    int *ts_n;
};
// stage clock for the latency breakdown: thread 0 of workgroup 0 appends s_memtime when a timestamp buffer is attached
__device__ __forceinline__ void fwd_stamp(const FwdLocal &loc) {
    if (loc.ts && blockIdx.x == 0 && threadIdx.x == 0) { const int i = *loc.ts_n; if (i < 4096) { loc.ts[i] = wall_clock64(); *loc.ts_n = i + 1; } }
}

template <bool WLDS>
__device__ __forceinline__ void flat_forward_core(const FlatArgs &a, float *lds, int wlds_row0, int sbase, const FwdLocal &loc) {
    float *HX = lds + FL_HX * LS, *H = lds + FL_H * LS, *G = lds + FL_G * LS, *C = lds + FL_C * LS, *X96 = lds + FL_X96 * LS,
          *T1 = lds + FL_T1 * LS, *T2 = lds + FL_T2 * LS, *ST = lds + FL_ST * LS, *SM = lds + FL_SM * LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = sbase + lane;
    const bool valid = s < a.n;
    const int ss = valid ? s : 0;
    const float *P = a.P;
    const int D = a.D, T = a.T, A = a.A, n = a.n;
    const WsOff wo = ws_offsets(T, A);
    float *ws = a.ws;
    const float *hrow = nullptr;
    int hstep = 0, nrows = loc.nrows, len = loc.len;
    const bool synth = loc.staged || (a.nhist != nullptr && a.wstride == 0);
    if (!loc.staged) {
        if (a.wstride) flat_lengths_win(a, ss, true, hrow, hstep, nrows, len);
        else flat_lengths(a, ss, true, hrow, hstep, nrows, len);
    }
    float *WG = lds + wlds_row0 * LS, *WC = WG + (D + FH) * 2 * FH;
    if (WLDS && !loc.weights_ready) {
        for (int i = tid; i < (D + FH) * 2 * FH; i += 256) WG[i] = P[a.o.gw + i];
        for (int i = tid; i < (D + FH) * FH; i += 256) WC[i] = P[a.o.cw + i];
    }
    for (int i = wave; i < FH; i += 4) H[i * LS + lane] = 0.f;
    if (!loc.staged)
        for (int i = wave; i < a.S0; i += 4) ST[i * LS + lane] = a.states[(long)ss * a.S0 + i];
    for (int t = 0; t < T; ++t) {
        // GRUCell (TF 1.4): r,u = sigmoid([x,h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u*h + (1-u)*c
        __syncthreads();
        if (synth)      // synthesized window (D == S0): the row is the current state, already staged in ST -- no global loads in the loop
            for (int i = wave; i < D; i += 4) HX[i * LS + lane] = t < nrows ? ST[i * LS + lane] : 0.f;
        else
            for (int i = wave; i < D; i += 4) HX[i * LS + lane] = t < nrows ? hrow[t * hstep + i] : 0.f;
        for (int i = wave; i < FH; i += 4) {
            const float hv = H[i * LS + lane];
            HX[(D + i) * LS + lane] = hv;
            if (ws && valid) ws_row(ws, ws_step(t) + i, sbase, wo.total)[lane] = hv;
        }
        __syncthreads();
        {
            const float *wg = WLDS ? WG : P + a.o.gw;
            float *wsg = ws ? ws_row(ws, ws_step(t) + FH, sbase, wo.total) : nullptr;
            // compile-time K only in the small-grid instance: its ~66 extra registers halve the occupancy of a full-size grid
            if (WLDS && D == 33) mm_fwd<65>(wg, 2 * FH, P + a.o.gb, HX, 65, 2 * FH, G, FACT_SIGMOID, wsg, n, sbase, wave, lane);
            else if (WLDS && D == 2) mm_fwd<34>(wg, 2 * FH, P + a.o.gb, HX, 34, 2 * FH, G, FACT_SIGMOID, wsg, n, sbase, wave, lane);
            else mm_fwd(wg, 2 * FH, P + a.o.gb, HX, D + FH, 2 * FH, G, FACT_SIGMOID, wsg, n, sbase, wave, lane);
        }
        __syncthreads();
        for (int i = wave; i < FH; i += 4) HX[(D + i) * LS + lane] = G[i * LS + lane] * H[i * LS + lane];
        __syncthreads();
        {
            const float *wc = WLDS ? WC : P + a.o.cw;
            float *wsc = ws ? ws_row(ws, ws_step(t) + 3 * FH, sbase, wo.total) : nullptr;
            if (WLDS && D == 33) mm_fwd<65>(wc, FH, P + a.o.cb, HX, 65, FH, C, FACT_TANH, wsc, n, sbase, wave, lane);
            else if (WLDS && D == 2) mm_fwd<34>(wc, FH, P + a.o.cb, HX, 34, FH, C, FACT_TANH, wsc, n, sbase, wave, lane);
            else mm_fwd(wc, FH, P + a.o.cb, HX, D + FH, FH, C, FACT_TANH, wsc, n, sbase, wave, lane);
        }
        __syncthreads();
        if (t < len)      // dynamic_rnn(sequence_length): the state is copied through past the end
            for (int i = wave; i < FH; i += 4) {
                const float u = G[(FH + i) * LS + lane];
                H[i * LS + lane] = u * H[i * LS + lane] + (1.0f - u) * C[i * LS + lane];
            }
    }
    __syncthreads();
    if (ws && valid)
        for (int i = wave; i < FH; i += 4) ws_row(ws, wo.hl + i, sbase, wo.total)[lane] = H[i * LS + lane];
    // rnn_graph_lstm (a3c/estimators.py:24-28): dense_temporal, dense_static x2, concat
    mm_fwd(P + a.o.tw, 2 * FH, P + a.o.tb, H, FH, 2 * FH, X96, FACT_RELU, ws ? ws_row(ws, wo.dt, sbase, wo.total) : nullptr, n, sbase, wave, lane);
    mm_fwd(P + a.o.s1w, 2 * FH, P + a.o.s1b, ST, a.S0, 2 * FH, T1, FACT_RELU, ws ? ws_row(ws, wo.s1, sbase, wo.total) : nullptr, n, sbase, wave, lane);
    __syncthreads();
    mm_fwd(P + a.o.s2w, FH, P + a.o.s2b, T1, 2 * FH, FH, X96 + 2 * FH * LS, FACT_RELU, ws ? ws_row(ws, wo.s2, sbase, wo.total) : nullptr, n, sbase, wave, lane);
    // mu / sigma heads (policy_v_network.py:214-226) -- two hidden layers each
    for (int head = 0; head < 2; ++head) {
        const long w1 = head ? a.o.g1w : a.o.m1w, b1 = head ? a.o.g1b : a.o.m1b, w2 = head ? a.o.g2w : a.o.m2w,
                   b2 = head ? a.o.g2b : a.o.m2b, w3 = head ? a.o.g3w : a.o.m3w, b3 = head ? a.o.g3b : a.o.m3b;
        const int o1 = head ? wo.g1 : wo.m1, o2 = head ? wo.g2 : wo.m2, o3 = head ? wo.sg : wo.tm;
        __syncthreads();
        mm_fwd(P + w1, 2 * FH, P + b1, X96, 3 * FH, 2 * FH, T1, FACT_RELU, ws ? ws_row(ws, o1, sbase, wo.total) : nullptr, n, sbase, wave, lane);
        __syncthreads();
        mm_fwd(P + w2, FH, P + b2, T1, 2 * FH, FH, T2, FACT_TANH, ws ? ws_row(ws, o2, sbase, wo.total) : nullptr, n, sbase, wave, lane);
        __syncthreads();
        mm_fwd(P + w3, A, P + b3, T2, FH, A, SM, head ? FACT_SIGMOID : FACT_TANH, ws ? ws_row(ws, o3, sbase, wo.total) : nullptr, n, sbase, wave, lane);
        __syncthreads();
        for (int k = wave; k < A; k += 4) {
            const float v = SM[k * LS + lane];
            const float out = head ? v + 1e-3f : a.bound * v;      // sigmoid(.) + 1e-3 (:223-226); ((ub-lb)/2)*tanh + (lb+ub)/2 with lb = -ub (:219)
            if (head) { if (valid && a.sigma) a.sigma[(long)s * A + k] = out; if (loc.SGL) loc.SGL[k * LS + lane] = out; }
            else { if (valid && a.mu) a.mu[(long)s * A + k] = out; if (loc.MUL) loc.MUL[k * LS + lane] = out; }
        }
    }
    // value head (:237-244): scale * Dense1(tanh(Dense64(x)))
    __syncthreads();
    mm_fwd(P + a.o.v1w, 2 * FH, P + a.o.v1b, X96, 3 * FH, 2 * FH, T1, FACT_TANH, ws ? ws_row(ws, wo.v1, sbase, wo.total) : nullptr, n, sbase, wave, lane);
    __syncthreads();
    mm_fwd(P + a.o.v2w, 1, P + a.o.v2b, T1, 2 * FH, 1, SM, FACT_NONE, nullptr, n, sbase, wave, lane);
    __syncthreads();
    if (wave == 0) {
        const float v = a.scale * SM[lane];
        if (valid && a.vs) a.vs[s] = v;
        if (loc.VSL) loc.VSL[lane] = v;
        if (ws && valid) ws_row(ws, wo.vs, sbase, wo.total)[lane] = v;
    }
}

template <bool WLDS>
__global__ __launch_bounds__(256) void flat_forward_kernel(FlatArgs a, int wlds_row0) {
    // WLDS = the small-grid instance (<= 256 workgroups, at most one per CU: LDS and registers to spare)
    extern __shared__ float lds[];
    FwdLocal loc{};
    flat_forward_core<WLDS>(a, lds, wlds_row0, blockIdx.x * 64, loc);
}

// ------------------------------------------------------------------------------------------ backward
constexpr int FB_C = 0;                  // d x96 (96); after the trunk its rows hold dL/dh (0..31) and KEEP (32..63)
constexpr int FB_A = FB_C + 96;          // forward inputs of the layer at hand (<= 65)
constexpr int FB_B = FB_A + 65;          // dz of the layer at hand (64)
constexpr int FB_T = FB_B + 64;          // dx of the layer at hand (<= 65)
constexpr int FB_DH = FB_C;              // dL/dh (32)
constexpr int FB_KEEP = FB_C + 32;       // part of dL/dh_prev that does not pass through the gate GEMM (32)
constexpr int FLAT_BWD_ROWS = FB_T + 65; // 290 rows = 75 KB: two workgroups per CU
constexpr int FLAT_LDS_ROWS = FLAT_BWD_ROWS > FLAT_FWD_ROWS ? FLAT_BWD_ROWS : FLAT_FWD_ROWS;
constexpr size_t FLAT_LDS_BYTES = (size_t)FLAT_LDS_ROWS * LS * sizeof(float);

__global__ __launch_bounds__(256, 2) void flat_backward_kernel(FlatArgs a) {
    extern __shared__ float lds[];
    float *bufC = lds + FB_C * LS, *bufA = lds + FB_A * LS, *bufB = lds + FB_B * LS, *bufT = lds + FB_T * LS,
          *DH = lds + FB_DH * LS, *KEEP = lds + FB_KEEP * LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *P = a.P;
    const int D = a.D, T = a.T, A = a.A, n = a.n;
    const WsOff wo = ws_offsets(T, A);
    const float *ws = a.ws;
    float *Gs = a.slab + (long)blockIdx.x * a.o.total;
    const int groups = (n + 63) / 64;
    float loss_p = 0.f, loss_c = 0.f;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int s = grp * 64 + lane;
        const bool valid = s < n;
        const int ss = valid ? s : 0;
        auto Wf = [&](int f) { return valid ? ws_row(ws, f, grp * 64, wo.total)[lane] : 0.f; };
        __syncthreads();
        // ---- loss terms (policy_v_network.py:228-251): mean over (n, A) of -logp*adv; mean over n of 0.25*(vs-y)^2/scale
        const float advs = valid ? a.adv[ss] : 0.f, tgt = valid ? a.y[ss] : 0.f, vsv = Wf(wo.vs);
        const float dlogp = -advs * a.inv_n / (float)A;
        const float dvs = valid ? 0.5f * (vsv - tgt) / a.scale * a.inv_n : 0.f;
        if (valid && wave == 0) loss_c += 0.25f * (vsv - tgt) * (vsv - tgt) / a.scale;
        // the 96 inputs of the three head layers (x96) are staged through bufA in two pieces when their weight gradient
        // is formed, instead of occupying 96 more LDS rows for the whole pass
        auto wgrad_x96 = [&](long w, long b) {
            for (int i = wave; i < 2 * FH; i += 4) bufA[i * LS + lane] = Wf(wo.dt + i);
            __syncthreads();
            mm_wgrad(bufA, bufB, 2 * FH, 2 * FH, Gs + w, Gs + b, wave, lane);
            __syncthreads();
            for (int i = wave; i < FH; i += 4) bufA[i * LS + lane] = Wf(wo.s2 + i);
            __syncthreads();
            mm_wgrad(bufA, bufB, FH, 2 * FH, Gs + w + 2 * FH * 2 * FH, Gs + b, wave, lane, false);
        };
        for (int head = 0; head < 2; ++head) {
            const long w1 = head ? a.o.g1w : a.o.m1w, b1 = head ? a.o.g1b : a.o.m1b, w2 = head ? a.o.g2w : a.o.m2w,
                       b2 = head ? a.o.g2b : a.o.m2b, w3 = head ? a.o.g3w : a.o.m3w, b3 = head ? a.o.g3b : a.o.m3b;
            const int o1 = head ? wo.g1 : wo.m1, o2 = head ? wo.g2 : wo.m2;
            __syncthreads();
            for (int k = wave; k < A; k += 4) {
                const float tm = Wf(wo.tm + k), sg = Wf(wo.sg + k);
                const float mu = a.bound * tm, sigma = sg + 1e-3f;
                const float act = valid ? a.actions[(long)ss * A + k] : mu;
                const float diff = act - mu;
                float dz;
                if (head == 0) {
                    dz = dlogp * diff / (sigma * sigma) * a.bound * (1.0f - tm * tm);
                    if (valid) loss_p += -(-0.5f * (diff / sigma) * (diff / sigma) - logf(sigma) - 0.9189385332046727f) * advs;
                } else {
                    dz = dlogp * (diff * diff / (sigma * sigma * sigma) - 1.0f / sigma) * sg * (1.0f - sg);
                }
                bufB[k * LS + lane] = valid ? dz : 0.f;
            }
            for (int i = wave; i < FH; i += 4) bufA[i * LS + lane] = Wf(o2 + i);
            __syncthreads();
            mm_wgrad(bufA, bufB, FH, A, Gs + w3, Gs + b3, wave, lane);
            mm_dx(P + w3, FH, A, bufB, bufT, false, wave, lane);
            __syncthreads();
            for (int i = wave; i < FH; i += 4) { const float m2 = bufA[i * LS + lane]; bufB[i * LS + lane] = bufT[i * LS + lane] * (1.0f - m2 * m2); }
            __syncthreads();
            for (int i = wave; i < 2 * FH; i += 4) bufA[i * LS + lane] = Wf(o1 + i);
            __syncthreads();
            mm_wgrad(bufA, bufB, 2 * FH, FH, Gs + w2, Gs + b2, wave, lane);
            mm_dx(P + w2, 2 * FH, FH, bufB, bufT, false, wave, lane);
            __syncthreads();
            for (int i = wave; i < 2 * FH; i += 4) bufB[i * LS + lane] = bufA[i * LS + lane] > 0.f ? bufT[i * LS + lane] : 0.f;
            __syncthreads();
            mm_dx(P + w1, 3 * FH, 2 * FH, bufB, bufC, head != 0, wave, lane);
            wgrad_x96(w1, b1);
        }
        // ---- value head
        __syncthreads();
        if (wave == 0) bufB[lane] = dvs * a.scale;
        for (int i = wave; i < 2 * FH; i += 4) bufA[i * LS + lane] = Wf(wo.v1 + i);
        __syncthreads();
        mm_wgrad(bufA, bufB, 2 * FH, 1, Gs + a.o.v2w, Gs + a.o.v2b, wave, lane);
        mm_dx(P + a.o.v2w, 2 * FH, 1, bufB, bufT, false, wave, lane);
        __syncthreads();
        for (int i = wave; i < 2 * FH; i += 4) { const float v1 = bufA[i * LS + lane]; bufB[i * LS + lane] = bufT[i * LS + lane] * (1.0f - v1 * v1); }
        __syncthreads();
        mm_dx(P + a.o.v1w, 3 * FH, 2 * FH, bufB, bufC, true, wave, lane);
        wgrad_x96(a.o.v1w, a.o.v1b);
        __syncthreads();
        // ---- trunk: bufC holds d x96 = [d dense_temporal (64), d dense_static (32)]
        for (int i = wave; i < FH; i += 4) bufB[i * LS + lane] = Wf(wo.s2 + i) > 0.f ? bufC[(2 * FH + i) * LS + lane] : 0.f;
        for (int i = wave; i < 2 * FH; i += 4) bufA[i * LS + lane] = Wf(wo.s1 + i);
        __syncthreads();
        mm_wgrad(bufA, bufB, 2 * FH, FH, Gs + a.o.s2w, Gs + a.o.s2b, wave, lane);
        mm_dx(P + a.o.s2w, 2 * FH, FH, bufB, bufT, false, wave, lane);
        __syncthreads();
        for (int i = wave; i < 2 * FH; i += 4) bufB[i * LS + lane] = bufA[i * LS + lane] > 0.f ? bufT[i * LS + lane] : 0.f;
        __syncthreads();
        for (int i = wave; i < a.S0; i += 4) bufA[i * LS + lane] = valid ? a.states[(long)ss * a.S0 + i] : 0.f;
        __syncthreads();
        mm_wgrad(bufA, bufB, a.S0, 2 * FH, Gs + a.o.s1w, Gs + a.o.s1b, wave, lane);
        __syncthreads();
        for (int i = wave; i < 2 * FH; i += 4) bufB[i * LS + lane] = Wf(wo.dt + i) > 0.f ? bufC[i * LS + lane] : 0.f;
        for (int i = wave; i < FH; i += 4) bufA[i * LS + lane] = Wf(wo.hl + i);
        __syncthreads();
        mm_wgrad(bufA, bufB, FH, 2 * FH, Gs + a.o.tw, Gs + a.o.tb, wave, lane);
        mm_dx(P + a.o.tw, FH, 2 * FH, bufB, DH, false, wave, lane);
        // ---- GRU, back through time with the sequence-length mask
        const float *hrow;
        int hstep, nrows, len;
        if (a.wstride) flat_lengths_win(a, ss, valid, hrow, hstep, nrows, len);
        else flat_lengths(a, ss, valid, hrow, hstep, nrows, len);
        for (int t = T - 1; t >= 0; --t) {
            const bool act = t < len;
            __syncthreads();
            for (int i = wave; i < D; i += 4) bufA[i * LS + lane] = (valid && t < nrows) ? hrow[t * hstep + i] : 0.f;
            for (int i = wave; i < FH; i += 4) {
                const float hp = Wf(ws_step(t) + i), r = Wf(ws_step(t) + FH + i), u = Wf(ws_step(t) + 2 * FH + i), c = Wf(ws_step(t) + 3 * FH + i);
                const float dhn = act ? DH[i * LS + lane] : 0.f;
                KEEP[i * LS + lane] = dhn * u;
                bufB[i * LS + lane] = dhn * (1.0f - u) * (1.0f - c * c);             // dz of the candidate
                bufB[(FH + i) * LS + lane] = dhn * (hp - c) * u * (1.0f - u);         // dz of the update gate (kept for later)
                bufA[(D + i) * LS + lane] = r * hp;
            }
            __syncthreads();
            mm_wgrad(bufA, bufB, D + FH, FH, Gs + a.o.cw, Gs + a.o.cb, wave, lane);
            mm_dx(P + a.o.cw, D + FH, FH, bufB, bufT, false, wave, lane);
            __syncthreads();
            for (int i = wave; i < FH; i += 4) {
                const float hp = Wf(ws_step(t) + i), r = Wf(ws_step(t) + FH + i);
                const float drh = bufT[(D + i) * LS + lane];
                KEEP[i * LS + lane] += drh * r;
                bufB[i * LS + lane] = drh * hp * r * (1.0f - r);                     // dz of the reset gate
                bufA[(D + i) * LS + lane] = hp;
            }
            __syncthreads();
            mm_wgrad(bufA, bufB, D + FH, 2 * FH, Gs + a.o.gw, Gs + a.o.gb, wave, lane);
            mm_dx(P + a.o.gw, D + FH, 2 * FH, bufB, bufT, false, wave, lane);
            __syncthreads();
            if (act)
                for (int i = wave; i < FH; i += 4) DH[i * LS + lane] = KEEP[i * LS + lane] + bufT[(D + i) * LS + lane];
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { loss_p += __shfl_xor(loss_p, d); loss_c += __shfl_xor(loss_c, d); }
    if (lane == 0) {
        atomicAdd(&a.stats64[0], (double)loss_p);
        atomicAdd(&a.stats64[1], (double)loss_c);
    }
}
