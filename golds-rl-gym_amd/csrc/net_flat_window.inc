// Included by net_flat.hip (inside namespace grl, after net_flat_eval.inc): the flat PAAC policy under the TRUE history window
// (grl_fnet_set_true_window, include/goldsrl_flatwindow.h).
//
// Window rule (SolowPolicyMonitor.eval_once, fed_gym/agents/paac/policy_monitor.py:84-108; a3c_window_step in net_a3c_core.inc): the
// last L = min(k + 1, rnn) processed states of the env's current episode, oldest first, the current state last, zero rows behind;
// k = steps since the episode's reset.  The worker's window (quirk Q11, emulator_runner.py:48-63) is L copies of the current state.
//
// Storage: no ring and no per-sample copy.  The rollout's state buffer has rnn - 1 leading time slices and one trailing slice for
// the bootstrap observation, (rnn - 1 + T + 1, E, S0) with ro_states at slice rnn - 1, so the window of sample (t, e) is a strided
// view: L rows E * S0 floats apart that end at ro_states[t][e].  FlatArgs describes it as {states, nhist = L per sample, wstride =
// E}: row j of sample ss is states + (ss + (j - L + 1) * wstride) * S0.  The general kernels (net_flat_mfma.inc: flat_lengths_win)
// train on these views; the forward below is the fast forward (net_flat_fast.inc) for them.  The evaluation, whose episodes have
// no bound a slab could be sized by, keeps a ring of wring = rnn slices: slice (t mod rnn) is step t's state.
//
// Forward with distinct rows.  The input halves x_t Wg[:D] and x_t Wc[:D] differ per row, so they cannot be formed once per forward
// as for the repeated row; a GRU stage is ONE chain of K = D + 32 per tile: the x_t products first (weights of the input half in
// registers, read once per forward; x_t from the slab in L2, requested one GRU step ahead so the load is off the dependent chain),
// then the eight recurrent products of ff_tile_reg32.  The GRU step stays two stages, the epilogues are those of
// flat_forward_fast.  The static branch and the heads do not see the window: the first stage here computes dense_static 1, and
// the heads are flat_forward_fast's own piece 3, the very instance the quirk-mode rollout calls.
// Two forms, one chain per sample: flat_forward_win_kernel (a launch per forward: the graph form of the rollout, predict_env) and
// the calls flat_forward_win_in / _rec (persistent rollout and evaluation); no piece needs callee-saved registers (LABNOTES F).

// the slice that holds row j of a window of L rows ending at step tcur
__device__ __forceinline__ const float *win_row(const FlatArgs &a, int tcur, int e, int L, int j) {
    int slice = tcur - (L - 1) + j;
    if (a.wring) slice %= a.wring;      // evaluation: L <= tcur + 1, so the slice is never negative
    return a.states + ((long)slice * a.wstride + e) * a.S0;
}

// per-sample ints of the forward, in rows the repeated-row form uses for XG (free here): the window's rows
__device__ __forceinline__ int *win_nrows(float *lds) { return reinterpret_cast<int *>(lds + FF_XG * LS); }

// step and env of sample s of the group: staged (persistent kernels) -- step wt, env sbase + s; otherwise sample sbase + s of a
// step-major batch of wstride envs per step
__device__ __forceinline__ void win_sample(const FlatArgs &a, bool staged, int wt, int sbase, int s, int &tcur, int &e) {
    if (staged) { tcur = wt; e = sbase + s; return; }
    const int gs = sbase + s;
    tcur = gs / a.wstride;
    e = gs - tcur * a.wstride;
}

// PART 1: the stage that needs only the inputs -- true_length of every window, dense_static 1.  L: the window's rows of the lane's
// sample (staged; otherwise a.nhist).  PART 2: the recurrence.  NQ = ceil(D / 4) k-steps of the input half (1: Solow, 9: D <= 33).
template <int G, int NQ, int PART>
__device__ __forceinline__ void flat_forward_win(const FlatArgs &a, float *lds, int sbase, bool staged, int L, int wt, const float (&wgr)[12],
                                                 const float (&wcr)[12]) {
    constexpr int NST = GroupTiles<G>::NST, SSH = GroupTiles<G>::SSH, SM = GroupTiles<G>::SM;
    [[maybe_unused]] float *H = lds + FF_H * LS, *X96 = lds + FF_X96 * LS, *RH = lds + FF_RH * LS, *U = lds + FF_U * LS, *S1 = lds + FF_S1 * LS,
          *ST = lds + FF_ST * LS;
    int *LENL = reinterpret_cast<int *>(ST + a.S0 * LS), *NRL = win_nrows(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *P = a.P;
    const int D = a.D, T = a.T, n = a.n;
    auto zero = [](int, int) { return 0.f; };
    if constexpr (PART == 1) {
        const bool own = lane < G && sbase + lane < n;
        if (!staged) {
            const int ss = own ? sbase + lane : 0;
            for (int i = wave; i < a.S0; i += FNW) ST[i * LS + lane] = a.states[(long)ss * a.S0 + i];
            L = a.nhist[ss];
        }
        L = L < 1 ? 1 : (L < T ? L : T);
        if (!own) L = 0;      // lanes without a sample read no row
        if (wave == 0) { NRL[lane] = L; LENL[lane] = 0; }
        for (int i = wave; i < FH; i += FNW) H[i * LS + lane] = 0.f;
        __syncthreads();
        // true_length (a3c/estimators.py:11-15): the rows with a non-zero entry, a row per wave
        L = NRL[lane];      // staged: only wave 0 was handed the rows
        int tcur, e;
        win_sample(a, staged, wt, sbase, lane, tcur, e);
        for (int j = wave; j < L; j += FNW) {
            const float *row = win_row(a, tcur, e, L, j);
            float m = 0.f;
            for (int i = 0; i < D; ++i) m = fmaxf(m, fabsf(row[i]));
            if (m > 0.f) atomicAdd(&LENL[lane], 1);
        }
#pragma nounroll
        for (int q = wave; q < 4 * NST; q += FNW)
            ff_tile_kd(P + a.o.s1w, 2 * FH, P + a.o.s1b, ST, a.S0, 2 * FH, (q >> SSH) * 16, (q & SM) * 16, lane, zero,
                       [&](int o, int s, float v) { S1[o * LS + s] = fmaxf(v, 0.f); });
        __syncthreads();
        // dense_static 2 for the groups whose piece 3 does not hold it (flat_forward_fast<G, false> has it in the first candidate stage:
        // there it cost the recurrence registers it has no room for next to two rows and the input halves' weights)
        if constexpr (NST >= 2) {
            if (wave < 2 * NST)
                ff_tile<2 * FH>(P + a.o.s2w, FH, P + a.o.s2b, S1, 2 * FH, FH, (wave >> SSH) * 16, (wave & SM) * 16, lane, zero,
                                [&](int o, int sq, float v) { X96[(2 * FH + o) * LS + sq] = fmaxf(v, 0.f); });
            __syncthreads();
        }
    }
    if constexpr (PART == 2) {
        const int lc = lane & 15, kq = lane >> 4;
        const bool tile_wave = wave < 4 * NST;
        const int s = (wave & SM) * 16 + lc, o0 = (wave >> SSH) * 16;
        const int ot = (wave >> SSH) & 3, og = ot * 16 + lc, ocn = (ot & 1) * 16 + lc;
        const int Ls = tile_wave ? NRL[s] : 0;
        int tcur, e;
        win_sample(a, staged, wt, sbase, s, tcur, e);
        // the input halves of the GRU kernels as A fragments: k = 4 j + kq
        float agx[NQ], acx[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int i = 4 * j + kq, ic = i < D ? i : D - 1;
            agx[j] = P[a.o.gw + (long)ic * 2 * FH + og];
            acx[j] = P[a.o.cw + (long)ic * FH + ocn];
            agx[j] = i < D ? agx[j] : 0.f;
            acx[j] = i < D ? acx[j] : 0.f;
        }
        // row t of the tile's sample as B fragments; zero rows behind the window's L
        auto load_row = [&](int t, float (&b)[NQ]) {
            const bool has = t < Ls;
            const float *row = has ? win_row(a, tcur, e, Ls, t) : a.states;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int i = 4 * j + kq;
                b[j] = (has && i < D) ? row[i] : 0.f;
            }
        };
        // [x_t, h] against the kernel's rows in the order of the concatenation: the input half, then ff_tile_reg32's chain
        auto tile = [&](const float (&ax)[NQ], const float (&bx)[NQ], const float (&av)[12], const float *X, auto epi) {
            f32x4f acc = {0.f, 0.f, 0.f, 0.f};
            float bv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = X[(4 * j + kq) * LS + s];
#pragma unroll
            for (int j = 0; j < NQ; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[j], bx[j], acc, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(o0 + 4 * kq + r, s, acc[r] + av[8 + r]);
        };
        float bx[NQ];
        load_row(0, bx);
#pragma nounroll
        for (int t = 0; t < T; ++t) {
            float bn[NQ];
            load_row(t + 1 < T ? t + 1 : T, bn);      // the next step's row: in flight across this step's two stages
            // GRUCell (TF 1.4): r,u = sigmoid([x,h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u*h + (1-u)*c
            if (tile_wave)
                tile(agx, bx, wgr, H, [&](int o, int sq, float v) {
                    v = sigmoidf_(v);
                    if (o < FH) RH[o * LS + sq] = v * H[o * LS + sq];
                    else U[(o - FH) * LS + sq] = v;
                });
            __syncthreads();
            if (wave < 2 * NST) {
                tile(acx, bx, wcr, RH, [&](int o, int sq, float v) {
                    v = tanhf(v);
                    if (t < LENL[sq]) {      // dynamic_rnn(sequence_length): the state is copied through past the end
                        const float u = U[o * LS + sq];
                        H[o * LS + sq] = u * H[o * LS + sq] + (1.0f - u) * v;
                    }
                });
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NQ; ++j) bx[j] = bn[j];
        }
    }
}

// the pieces as calls from the persistent kernels (the argument block in the net's constant-memory slot, as flat_forward_fast_part)
template <int G, int NQ>
__device__ __noinline__ void flat_forward_win_in(int slot, float *lds, int sbase, int L, int wt) {
    const FlatArgs &a = g_flat_args[__builtin_amdgcn_readfirstlane(slot)];
    const float none[12] = {};
    flat_forward_win<G, NQ, 1>(a, lds, sbase, true, L, __builtin_amdgcn_readfirstlane(wt), none, none);
}
template <int G, int NQ>
__device__ __noinline__ void flat_forward_win_rec(int slot, float *lds, int sbase, int wt, f32x4f g0, f32x4f g1, f32x4f g2, f32x4f c0, f32x4f c1,
                                                  f32x4f c2) {
    const FlatArgs &a = g_flat_args[__builtin_amdgcn_readfirstlane(slot)];
    const float wg[12] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3], g2[0], g2[1], g2[2], g2[3]};
    const float wc[12] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3], c2[0], c2[1], c2[2], c2[3]};
    flat_forward_win<G, NQ, 2>(a, lds, sbase, true, 0, __builtin_amdgcn_readfirstlane(wt), wg, wc);
}
// the whole forward of step wt for the group; L: the window's rows of the lane's env.  Ends on a barrier (piece 3's).
template <int G>
__device__ __forceinline__ void flat_forward_win_call(int slot, float *lds, int sbase, int L, int wt, bool small_d, const RecW &w) {
    const f32x4f g0{w.g[0], w.g[1], w.g[2], w.g[3]}, g1{w.g[4], w.g[5], w.g[6], w.g[7]}, g2{w.g[8], w.g[9], w.g[10], w.g[11]};
    const f32x4f c0{w.c[0], w.c[1], w.c[2], w.c[3]}, c1{w.c[4], w.c[5], w.c[6], w.c[7]}, c2{w.c[8], w.c[9], w.c[10], w.c[11]};
    if (small_d) {
        flat_forward_win_in<G, 1>(slot, lds, sbase, L, wt);
        flat_forward_win_rec<G, 1>(slot, lds, sbase, wt, g0, g1, g2, c0, c1, c2);
    } else {
        flat_forward_win_in<G, 9>(slot, lds, sbase, L, wt);
        flat_forward_win_rec<G, 9>(slot, lds, sbase, wt, g0, g1, g2, c0, c1, c2);
    }
    flat_forward_fast_part<G, false, 3>(slot, lds, sbase, 0, -1);
}

// one launch per forward over windows in global memory: a.states / a.nhist / a.wstride (no ring), outputs a.mu / a.sigma / a.vs
template <int NQ>
__global__ __launch_bounds__(FNT) void flat_forward_win_kernel(FlatArgs a) {
    extern __shared__ float lds[];
    FwdLocal loc{};
    float wgr[12], wcr[12];
    ff_load_recurrent<64>(a, wgr, wcr);
    const int sbase = blockIdx.x * 64;
    flat_forward_win<64, NQ, 1>(a, lds, sbase, false, 0, 0, wgr, wcr);
    flat_forward_win<64, NQ, 2>(a, lds, sbase, false, 0, 0, wgr, wcr);
    flat_forward_fast<64, false, true, 3>(a, lds, sbase, loc, wgr, wcr);
}

// ------------------------------------------------------------------------------------------ window state between calls
// the last `lead` slices of the previous rollout (or of an older buffer) to the front of the slab.  A thread owns one float of a
// slice and walks the slices in ascending order: src lies behind dst, so inside one buffer this is a shift (T < rnn - 1 included)
__global__ void flat_window_carry_kernel(const float *src, float *dst, int lead, long slice) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= slice) return;
    for (int j = 0; j < lead; ++j) dst[(long)j * slice + i] = src[(long)j * slice + i];
}

// windows restart (the current observation alone) for every env when `all`, else for the envs whose TimeLimit counter or episode
// number is not what the net left behind: the host reset or stepped them, and the net has not seen the states in between
__global__ void flat_window_detect_kernel(int32_t *wlen, const int32_t *elapsed, const int32_t *episode, const int32_t *seen_elapsed,
                                          const int32_t *seen_episode, int E, int all) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (all || elapsed[e] != seen_elapsed[e] || episode[e] != seen_episode[e] || wlen[e] < 1) wlen[e] = 1;
}

// graph form, behind the env step: the new state joins the window, or the window restarts on done
__global__ void flat_window_step_kernel(int32_t *wlen, const uint8_t *done, int E, int rnn) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int l = wlen[e] + 1;
    wlen[e] = done[e] ? 1 : (l < rnn ? l : rnn);
}

// dense (count, rnn, D) windows of samples [first, first + count) of a step-major batch: the indexing of flat_lengths_win
__global__ void flat_window_gather_kernel(const float *states, const int32_t *nhist, int wstride, int first, int count, int rnn, int D,
                                          float *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)count * rnn * D) return;
    const int c = (int)(i % D), j = (int)((i / D) % rnn), ss = first + (int)(i / ((long)D * rnn));
    int L = nhist[ss];
    L = L < 1 ? 1 : (L < rnn ? L : rnn);
    out[i] = j < L ? states[((long)ss + (long)(j - L + 1) * wstride) * D + c] : 0.f;
}

// ------------------------------------------------------------------------------------------ persistent rollout, true window
// all waves: the window's rows for the forward that follows (wave 0 first moves the window on behind the step before), states[t]
// into the slab -- the bootstrap observation too, slice T -- and nhist[t] = the rows
__device__ __noinline__ int ro_record_win(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    int *WL = reinterpret_cast<int *>(lds + R.off_wl);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = R.f.n, S0 = R.f.S0, Rn = R.f.T;
    int wl = 0;
    if (wave == 0) {
        wl = WL[lane];
        if (t > 0) { wl = L.DN[lane] ? 1 : (wl + 1 < Rn ? wl + 1 : Rn); WL[lane] = wl; }
        if (t < R.steps && ro_env(R, sbase, lane) < E) R.ro_nhist[(size_t)t * E + sbase + lane] = wl;
    }
    for (int idx = tid; idx < R.gs * S0; idx += FNT) {
        const int sl = idx / S0, i = idx - sl * S0;
        if (sbase + sl < E) R.ro_states[((size_t)t * E + sbase + sl) * S0 + i] = L.ST[i * LS + sl];
    }
    return wl;
}

template <int G>
__global__ __launch_bounds__(FNT) void flat_rollout_win_kernel(int slot) {
    const RolloutArgs &R = g_ro_args[slot];
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sbase = blockIdx.x * G, steps = R.steps;
    const int env = lane < G ? sbase + lane : 0x7fffffff;
    const bool valid = env < R.f.n;
    const bool solow = R.env_kind == GRL_ENV_SOLOW, small_d = R.f.D <= 4;
    int *WL = reinterpret_cast<int *>(lds + R.off_wl);
    RecW w;
    ff_load_recurrent<G>(R.f, w.g, w.c);
    ro_enter(slot, lds, sbase);
    if (wave == 0) WL[lane] = valid ? R.wlen[env] : 1;
    __syncthreads();
    const uint32_t counter0 = *R.counter_base;
    for (int t = 0; t <= steps; ++t) {
        const int wl = ro_record_win(slot, lds, t, sbase);
        flat_forward_win_call<G>(R.slot, lds, sbase, wl, t, small_d, w);      // its first barrier stands between the slab's stores and loads
        if (t == steps) break;      // that was the bootstrap forward: the window behind the last step
        ro_sample(slot, lds, t, sbase, counter0 + (uint32_t)t);
        __syncthreads();
        if (!solow) {
            ro_trade_trades(slot, lds, lane, wave, env, valid);
            __syncthreads();
        }
        if (solow) {
            if (wave == 0) ro_solow_env_step(slot, lds, t, sbase);
        } else {
            ro_trade_step(slot, lds, t, sbase);
        }
        __syncthreads();
        if (solow && R.needs_tape) {
            const int *DN = reinterpret_cast<int *>(lds + R.row_int * LS) + LS;
            const unsigned long long m = __ballot(DN[lane] != 0);
            if (m) {
                ro_solow_tapes(slot, lds, m, sbase);
                __syncthreads();
            }
        }
    }
    if (wave == 0 && valid) {
        R.wlen[env] = WL[lane];      // the rows the next rollout's first step sees, its own observation included
        ro_returns(slot, lds, lane, env);
    }
    if (!solow) ro_leave_trade(slot, lds, sbase);
}

// ------------------------------------------------------------------------------------------ evaluation, true window
// all waves: as ev_record; the state of step t goes to slice t mod rnn of the ring, the window grows by the state (an env that
// is done plays no more: its window is never read again)
__device__ __noinline__ int ev_record_win(int slot, float *lds, int t, int sbase) {
    RO_ARGS(slot);
    const RoLds L = ro_lds(R, lds);
    int *WL = reinterpret_cast<int *>(lds + R.off_wl);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = R.f.n, S0 = R.f.S0, Rn = R.f.T;
    float *ring = const_cast<float *>(R.f.states) + (size_t)(t % R.f.wring) * E * S0;
    const bool trace = t < R.ev.trace_steps;
    int wl = 0;
    if (wave == 0) {
        wl = WL[lane];
        if (t > 0) { wl = wl + 1 < Rn ? wl + 1 : Rn; WL[lane] = wl; }
        if (trace && ro_env(R, sbase, lane) < E && L.DN[lane] == 0) R.ev.nhist[(size_t)t * E + sbase + lane] = wl;
    }
    for (int idx = tid; idx < R.gs * S0; idx += FNT) {
        const int sl = idx / S0, i = idx - sl * S0;
        if (sbase + sl >= E) continue;
        const float v = L.ST[i * LS + sl];
        ring[(size_t)(sbase + sl) * S0 + i] = v;
        if (trace && L.DN[sl] == 0) R.ev.states[((size_t)t * E + sbase + sl) * S0 + i] = v;
    }
    return wl;
}

template <int G>
__global__ __launch_bounds__(FNT) void flat_eval_win_kernel(int slot, int live_off) {
    const RolloutArgs &R = g_ro_args[slot];
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sbase = blockIdx.x * G, max_steps = R.ev.max_steps;
    const int env = lane < G ? sbase + lane : 0x7fffffff;
    const bool valid = env < R.f.n;
    const bool solow = R.env_kind == GRL_ENV_SOLOW, small_d = R.f.D <= 4;
    const int *DN = reinterpret_cast<int *>(lds + R.row_int * LS) + LS;
    int *LIVE = reinterpret_cast<int *>(lds + live_off), *WL = reinterpret_cast<int *>(lds + R.off_wl);
    RecW w;
    ff_load_recurrent<G>(R.f, w.g, w.c);
    ro_enter(slot, lds, sbase);
    if (wave == 0) WL[lane] = 1;      // an evaluation starts every window at the observation it is entered with
    __syncthreads();
    const uint32_t counter0 = *R.counter_base;
    double total = 0.0;
    int len = 0;
#pragma unroll 1
    for (int t = 0; t < max_steps; ++t) {
        const int wl = ev_record_win(slot, lds, t, sbase);
        const int alive = (valid && DN[lane] == 0) ? 1 : 0;
        flat_forward_win_call<G>(R.slot, lds, sbase, wl, t, small_d, w);
        ev_sample(slot, lds, t, sbase, counter0 + (uint32_t)t, alive);
        __syncthreads();
        StepOut so{0.f, 0};
        if (solow) {
            if (wave == 0) so = ev_solow_env_step(slot, lds, t, sbase, alive);
        } else {
            ro_trade_trades(slot, lds, lane, wave, env, alive != 0);
            __syncthreads();
            so = ev_trade_step(slot, lds, t, sbase, alive);
        }
        if (wave == 0) {
            if (alive) { total += (double)so.reward; ++len; }
            const unsigned long long m = __ballot(alive && !so.done);
            if (lane == 0) *LIVE = m != 0ull ? 1 : 0;
        }
        __syncthreads();
        if (*LIVE == 0) break;
    }
    if (wave == 0 && valid) {
        R.ev.total[env] = total;
        R.ev.length[env] = len;
        R.ev.finished[env] = DN[lane] != 0 ? 1 : 0;
    }
}
