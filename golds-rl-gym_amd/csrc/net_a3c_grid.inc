// The softmax-grid head the A3C savings-grid agent (net_discrete.hip) and the grid trader (net_gridtrade.hip) share: the reference's
// DiscretePolicyEstimator (fed_gym/agents/a3c/estimators.py:18-28,155-238,338-417) with num_outputs = GRID_O.  Included behind
// net_a3c_core.inc inside namespace grl, the way the core is; the including file sets first
//   GRID_D      the processed observation, S0 = D (2 on Solow, 5 on a 2-asset TradeAR1)
//   GRID_O      the outputs (1, 2): one softmax over K grid points each
//   GRID_KMAX   the most grid points per output (64, 48)
//   GRID_RS     the Philox stream of the action draw (RS_GRID_ACTION, RS_GRIDTRADE_ACTION)
// and keeps its two __global__ kernels as wrappers around grid_forward / grid_backward, and its own evaluation kernel.
//   logits   ONE probs tower with N = O * K output rows; column o * K + j of probs3 is output o, choice j (the row-major reshape
//            (-1, O, K) of the reference), so output o's logits are the K rows at o * K of the dL/dx rows (L_DX, 96 rows).  They do
//            not fit the 16 head rows of the shared layout, and the layout does not grow: the dL/dx rows are free in the forward,
//            and in the backward free until the tower's last mm_dx writes them -- by then the weight gradient and the in-place dx
//            of layer 3 have consumed the logits' dz.  The value head stays in the O rows.
//   head     wave o owns output o, one lane per sample: softmax, cumulative-sum draw or arg-max, grid value, and in the backward the
//            loss terms and the logits' dz in place.  The outputs run at the same time on waves 0 .. O-1; the other waves wait at
//            the barrier.  Nothing of one output is read by another's wave.  What only wave 0 does (the value loss, the weight sum)
//            is written under wave == 0 inside wave < GRID_O, so that with O = 1 the code is the one-output net's.

// ---- the towers on the trunk's x.  They restate net_gauss.hip's gauss_tower_fwd / gauss_tower_bwd and its value head with the
// second layer's activation and the head's rows as parameters; the Gaussian net keeps its own, because routing it through these
// changed its kernels' code (DESIGN section 3).
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

constexpr int L_LG = L_DX;    // logits -> probs -> their dz: output o at rows o * K
static_assert(GRID_O * GRID_KMAX <= NX, "the logit rows overflow the dL/dx rows");

struct GridOff {
    long gw, gb, cw, cb, tw, tb, s1w, s1b, s2w, s2b, p1w, p1b, p2w, p2b, p3w, p3b, v1w, v1b, v2w, v2b, total;
};

static GridOff grid_offsets(int K) {
    GridOff o;
    long p = 0;
    auto take = [&](long n) { long r = p; p += n; return r; };
    o.gw = take((GRID_D + NH) * 2 * NH); o.gb = take(2 * NH); o.cw = take((GRID_D + NH) * NH); o.cb = take(NH);
    o.tw = take(NH * 2 * NH); o.tb = take(2 * NH); o.s1w = take(GRID_D * 2 * NH); o.s1b = take(2 * NH); o.s2w = take(2 * NH * NH); o.s2b = take(NH);
    o.p1w = take(NX * NW1); o.p1b = take(NW1); o.p2w = take(NW1 * NW2); o.p2b = take(NW2); o.p3w = take(NW2 * GRID_O * K); o.p3b = take(GRID_O * K);
    o.v1w = take(NX * NW1); o.v1b = take(NW1); o.v2w = take(NW1); o.v2b = take(1);
    o.total = p;
    return o;
}

struct GridArgs {
    const float *P;
    GridOff o;
    int n, R, K;
    float scale;
    double lb, ub;                      // the grid's ends
    const float *states, *win;          // (n,D) (n,R,D)
    const float *gate;                  // (n) or null: only samples with gate != 0 are evaluated (the terminal value pass)
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
    double *stats64;                    // policy loss, value loss, weighted entropy sum (over the outputs), weight sum
};

// what the evaluation kernels take (net_discrete_eval.inc, net_gridtrade_eval.inc)
struct GridEvalArgs {
    GridArgs a;                         // P, o, n = E, R, K; states = the handle's processed observation (E,D), win = the net's windows
    float *win;                         // (E,R,D), the same buffer as a.win
    float *act;                         // (E,O) the actions each env is stepped with
    int max_steps, trace_steps;
    double *total;                      // (E)
    int32_t *length;                    // (E)
    uint8_t *finished;                  // (E)
    float *tr_states, *tr_act, *tr_rew, *tr_done;      // (trace_steps, E, ..) or null
    int32_t *tr_choice;
};

template <bool LOOP>
__device__ __forceinline__ void grid_probs_fwd(const GridArgs &a, float *lds) {
    a3c_tower3_fwd<LOOP, FACT_RELU>(a.P, lds, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, GRID_O * a.K, lds + L_LG * LS);
}

// ---- the head of ONE output, one lane per sample: column `lane` of the K rows at PR = the output's first logit row (stride
// LS = 65: conflict-free down a column).  Sequential float32 arithmetic in index order, one operation per statement
// (-ffp-contract=off).
// tf.nn.softmax over the last axis of (n, O, K), in place: max-subtracted, the sum in index order
__device__ __forceinline__ void grid_softmax(float *PR, int K, int lane) {
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

// get_random_discrete_action (worker.py:223-227) per output: (u < cum_probs).argmax() -- the first j with u < the float32
// cumulative sum, 0 if none
__device__ __forceinline__ int grid_choose(const float *PR, int K, int lane, double u) {
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
__device__ __forceinline__ int grid_greedy(const float *PR, int K, int lane) {
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
__host__ __device__ inline float grid_value(int ch, int K, double lb, double ub) {
    const double step = (ub - lb) / (double)(K - 1);
    return (float)(ch == K - 1 ? ub : lb + (double)ch * step);
}

// what wave o < GRID_O does when the net acts for sample s: output o's choice
__device__ __forceinline__ int grid_act(const GridArgs &a, const float *PRo, int o, int lane, int s) {
    if (a.greedy) return grid_greedy(PRo, a.K, lane);
    double u0, u1;      // one Philox block per (env, step): its first uniform serves output 0, its second output 1
    u01_pair(rng_block(a.seed, (uint32_t)s + a.env_off, a.counter, GRID_RS, 0u), u0, u1);
    return grid_choose(PRo, a.K, lane, o == 0 ? u0 : u1);
}

// one launch per forward pass (predict, a rollout step, the bootstraps); with a.act: the draws or the arg-maxes and the grid
// values.  A pass that asks for values only (the bootstraps) skips the probs tower.
//
// TEACH (a second instantiation, the grid trader's teach rollout; GridNoTeach: the kernel as it always was): while waves 0 .. O-1
// run their heads, wave 2 + o computes tt.teacher(o, s), output o's teacher action for env s, and leaves it in row 1 + o of the O
// rows (free until the value head, which writes row 0 behind a barrier).  Behind the barrier wave o hands its own grid value and
// the teacher's action to tt.mix, which says what the env is stepped with.
struct GridNoTeach { static constexpr bool on = false; };
template <typename TEACH = GridNoTeach>
__device__ __forceinline__ void grid_forward(GridArgs a, float *lds, const TEACH &tt = TEACH()) {
    constexpr bool teach = TEACH::on;
    static_assert(!teach || 2 * GRID_O <= 4, "the teacher needs a wave per output beside the heads'");
    float *O = lds + L_O * LS, *PR = lds + L_LG * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sbase = blockIdx.x * 64, s = sbase + lane, K = a.K, OK = GRID_O * K;
    const bool valid = s < a.n;
    bool on = valid;
    if (a.gate) {      // every wave sees the same 64 samples: the exit is uniform over the workgroup
        on = valid && a.gate[s] != 0.f;
        if (__ballot(on) == 0ull) return;
    }
    a3c_trunk<GRID_D, GRID_D, false>(a, lds, sbase, nullptr);
    if (a.probs || a.act) {      // uniform: the bootstraps ask for values only
        grid_probs_fwd<false>(a, lds);
        float *PRo = PR + (wave < GRID_O ? wave : 0) * K * LS;
        if (wave < GRID_O) grid_softmax(PRo, K, lane);
        if constexpr (teach) {
            if (a.act && valid && wave >= 2 && wave < 2 + GRID_O) O[(wave - 1) * LS + lane] = tt.teacher(a, wave - 2, s);
        }
        __syncthreads();
        if (a.probs) {           // (n,O,K): the group's rows are contiguous and row o * K + j is element (o, j): coalesced
            const int cnt = (a.n - sbase < 64 ? a.n - sbase : 64) * OK;
            for (int i = threadIdx.x; i < cnt; i += 256) {
                const int sl = i / OK, j = i - sl * OK;
                a.probs[(size_t)sbase * OK + i] = PR[j * LS + sl];
            }
        }
        if (a.act && valid && wave < GRID_O) {
            const int ch = grid_act(a, PRo, wave, lane, s);
            a.choice_out[(size_t)s * GRID_O + wave] = ch;
            const float own = grid_value(ch, K, a.lb, a.ub);
            if constexpr (teach) a.act[(size_t)s * GRID_O + wave] = tt.mix(a, own, O[(wave + 1) * LS + lane], s);
            else a.act[(size_t)s * GRID_O + wave] = own;
        }
    }
    if (a.vals) {                // uniform
        a3c_value_fwd<false>(a, lds);
        if (on && wave == 0) a.vals[s] = a.scale * O[lane];
    }
}

// Losses (estimators.py:206-212, 377-378), per sample with coefficient c = grad_mult * weight and cp = c * adv:
//   policy  cp * sum_o -log(p_{o,ch_o} + 1e-7);  dz_{o,j} = cp * p_{o,ch_o} / (p_{o,ch_o} + 1e-7) * (p_{o,j} - [j == ch_o])
//   value   c * 0.5 * (v - target)^2 / scale,  v = scale * value2(...)
//   entropy the mean over o of -sum_j p_{o,j} log(p_{o,j} + 1e-7) (estimators.py:206), reported only
// The forward is recomputed per 64-sample group; with a single policy tower nothing is parked in scratch.  Wave o sums output o's
// terms and writes its dz in place; wave 0 also the value loss.  The workgroup loops over groups blockIdx.x, + gridDim.x, ..; its
// slab holds [policy P | value P] (cleared by the caller), reduced in a fixed order (no float atomics on gradients).
//
// TEACH (a second instantiation, the supervised update): the head's gradient is the cross-entropy to a soft label on the grid, mass
// y_lo = 1 - w on point lo and y_hi = w on lo + 1, with no advantage:
//   policy  c * sum_o -(y_lo log(p_lo + 1e-7) + y_hi log(p_hi + 1e-7));  with r_k = y_k * p_k / (p_k + 1e-7):
//           dz_{o,j} = c * (p_{o,j} * (r_lo + r_hi) - r_j).  A term with y_k = 0 is skipped: 0 * log never appears.
// Value loss, entropy and the reduction are the same statements.  Agreement: the weighted count of (sample, output) pairs whose
// arg-max (grid_greedy) is the label's heavier point, lo on a tie, summed into tl.agree.
struct GridLabels {
    const int32_t *lo;                  // (n,O) in [0, K - 2]
    const float *w;                     // (n,O) in [0, 1]
    double *agree;                      // (1), cleared by the caller
};
template <bool TEACH = false>
__device__ __forceinline__ void grid_backward(GridArgs a, float *lds, GridLabels tl = GridLabels{}) {
    float *O = lds + L_O * LS, *PR = lds + L_LG * LS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = a.K;
    const long Pn = a.o.total;
    float *Gp = a.slab + (size_t)blockIdx.x * 2 * Pn, *Gv = Gp + Pn;
    float *scr = a.scratch + (size_t)blockIdx.x * a3c_scratch_trunk_rows(a.R) * 64;
    const int groups = (a.n + 63) / 64;
    double lp = 0.0, lv = 0.0, ent = 0.0, wsum = 0.0, agree = 0.0;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int sbase = grp * 64, s = sbase + lane;
        const bool valid = s < a.n;
        const int ss = valid ? s : 0;
        const float wt = valid ? (a.wt ? a.wt[ss] : 1.0f) : 0.f;
        const float c = a.mult * wt, adv = TEACH ? 1.0f : a.adv[ss], cp = c * adv;
        const int len = a3c_length(a.win + (size_t)ss * a.R * GRID_D, a.R, GRID_D);
        a3c_trunk<GRID_D, GRID_D, true>(a, lds, sbase, scr);
        // ---- probs tower: each output's dz over its own probabilities, in place, on its own wave
        grid_probs_fwd<true>(a, lds);
        if (wave < GRID_O) {
            float *PRo = PR + wave * K * LS;
            grid_softmax(PRo, K, lane);
            if constexpr (TEACH) {
                int lo = tl.lo[(size_t)ss * GRID_O + wave];
                lo = lo < 0 ? 0 : (lo > K - 2 ? K - 2 : lo);      // the host checks its samples; the rollout's are in range
                const float w = tl.w[(size_t)ss * GRID_O + wave], ylo = 1.0f - w;
                const float plo = PRo[lo * LS + lane], phi = PRo[(lo + 1) * LS + lane];
                const bool on_lo = ylo > 0.f, on_hi = w > 0.f;
                const float rlo = on_lo ? ylo * (plo / (plo + 1e-7f)) : 0.f, rhi = on_hi ? w * (phi / (phi + 1e-7f)) : 0.f, rs = rlo + rhi;
                const int top = grid_greedy(PRo, K, lane);
                float h = 0.f;
                for (int j = 0; j < K; ++j) {
                    const float p = PRo[j * LS + lane];
                    h += p * logf(p + 1e-7f);
                    const float pr = p * rs;
                    PRo[j * LS + lane] = c * (pr - (j == lo ? rlo : (j == lo + 1 ? rhi : 0.f)));
                }
                if (valid && wt != 0.f) {      // weight-0 samples add nothing
                    float ce = 0.f;
                    if (on_lo) ce += ylo * logf(plo + 1e-7f);
                    if (on_hi) ce += w * logf(phi + 1e-7f);
                    lp += (double)(c * -ce);
                    ent += (double)wt * (double)(-h);
                    if (top == (w > 0.5f ? lo + 1 : lo)) agree += (double)wt;
                    if (wave == 0) wsum += (double)wt;
                }
            } else {
                int ch = a.choice[(size_t)ss * GRID_O + wave];
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
        }
        a3c_tower3_bwd<FACT_RELU>(a.P, lds, Gp, a.o.p1w, a.o.p1b, a.o.p2w, a.o.p2b, a.o.p3w, a.o.p3b, GRID_O * K, PR, false);
        a3c_trunk_bwd<GRID_D, GRID_D, true>(a, lds, sbase, scr, Gp, len);
        // ---- value head
        a3c_value_fwd<true>(a, lds);
        if (wave == 0) {
            const float v = a.scale * O[lane], tg = a.tgt[ss], dv = v - tg;
            O[lane] = c * dv;                               // d/dz of c * 0.5 (scale z - t)^2 / scale
            if (valid) lv += (double)(c * 0.5f * dv * dv / a.scale);
        }
        a3c_value_bwd(a, lds, Gv, wave, lane);
        a3c_trunk_bwd<GRID_D, GRID_D, true>(a, lds, sbase, scr, Gv, len);
    }
    // wave o < GRID_O summed output o's terms; wave 0 also the value loss and the weights
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lp += __shfl_xor(lp, d); lv += __shfl_xor(lv, d); ent += __shfl_xor(ent, d); wsum += __shfl_xor(wsum, d);
    }
    if (lane == 0 && wave < GRID_O) {
        atomicAdd(&a.stats64[0], lp);
        atomicAdd(&a.stats64[2], ent);
        if (wave == 0) { atomicAdd(&a.stats64[1], lv); atomicAdd(&a.stats64[3], wsum); }
    }
    if constexpr (TEACH) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) agree += __shfl_xor(agree, d);
        if (lane == 0 && wave < GRID_O) atomicAdd(tl.agree, agree);
    }
}
