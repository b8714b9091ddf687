// ConvPolicyVFieldNetwork acting and learning on a Swarm handle (include/goldsrl_fieldrollout.h); included by net_field.hip.
//
// The ten agents of an env see ONE (G, G, 2) density image, so the trunk -- convs, dense stack, pol2, value tower -- runs once per
// env and an agent only reads its 2A columns of the mu / sigma fields against the env's shared p2.
//   step (fused):  field_fused_step: one workgroup per env -- image from the 200-byte compact observation into LDS, conv+pool x L,
//                  dense stack, pol2, value tower out of LDS, the ten agents' head columns, a = mu + sigma N(0,1), norm clip, the
//                  observation record -- then the Swarm range step, the bookkeeping and the reward layout
//   step (layers): field_grid -> field_conv_pool / field_dense with N = envs (chunks of max_samples) -> field_heads_env (sample n
//                  reads row n / 10) -> field_sample.  The parent's arithmetic; GRL_FIELD_FUSED=off, or an env past 64 KB of LDS.
//   update:        per chunk of (t, env) samples the trunk is recomputed from the recorded compact observations (50 words per
//                  sample against ~3.4 K floats of activations), fr_heads_bwd sums the agents' d p2 / d z_v in agent order,
//                  fr_heads_wgrad walks the recorded positions listed per grid cell in (t, env, agent) order, and every weight gradient
//                  below the heads is split over the samples into slabs that are added in order.  No float atomics anywhere.
// Both head matrices are kept a second time column-major (muwt / sgwt [HWA][P2]): a column is then one contiguous run instead of
// 2HWA elements HWA*4 bytes apart.  The copies follow net->param_version.
#include <stdlib.h>

namespace grl {

enum : uint32_t { RS_FIELD_ACTION = 16 };      // the conv rollout's keying (net_conv.hip: RS_ACTION)
constexpr int FR_AGENTS = N_AGENTS;
constexpr int FR_A = 2;                        // SwarmEnv.step takes (10, 2) actions
constexpr int FR_DZ = 2 * FR_A + 3;            // a dzh row, as field_heads_bwd_kernel writes it
constexpr int FR_SPLIT = 128;                  // samples per slab of a split weight gradient
constexpr int FR_KT = 8;                       // rows of a dense weight gradient per lane
constexpr size_t FR_LDS_BYTES = 64 * 1024;

// the outputs of the last grl_fieldnet_eval (net_field_eval.inc); the buffers are on the handle's allocation list (episode_reserve)
struct FieldEval {
    double *rewards = nullptr, *actions = nullptr;                                       // (cap_steps) (cap_act,10,2)
    int32_t *length = nullptr;                                                          // (cap_envs)
    uint8_t *finished = nullptr;
    float *tr_mu = nullptr, *tr_sigma = nullptr, *tr_value = nullptr, *tr_raw = nullptr; // (cap_trace,10,2) x2, (cap_trace), (cap_trace,10,2)
    uint8_t *tr_lb = nullptr, *tr_ab = nullptr, *tr_pos = nullptr;                       // (cap_trace,80,2) (cap_trace,10,2) x2
    double *tr_x = nullptr, *tr_xa = nullptr;                                           // (cap_trace,80,2) (cap_trace,10,2)
    size_t cap_steps = 0, cap_act = 0, cap_envs = 0, cap_trace = 0;
    int max_steps = 0, trace_env = -1, keep_actions = 0;                                // of the last call; max_steps == 0: none yet
};

struct FieldRollout {
    int fused = -1;               // -1: environment not read yet
    bool headt = true;
    float gamma = 0.99f;
    long headt_version = -1;
    float *muwt = nullptr, *sgwt = nullptr;
    size_t lds_bytes = 0;
    int m0n = 0, m1n = 0;
    float *cur_mu = nullptr, *cur_sg = nullptr, *cur_vs = nullptr;      // predict_swarm / the bootstrap forward
    int T = 0, cap_T = 0;
    uint8_t *ro_lb = nullptr, *ro_ab = nullptr, *ro_pos = nullptr, *ro_done = nullptr;
    float *ro_act = nullptr, *ro_envact = nullptr, *ro_mu = nullptr, *ro_sg = nullptr, *ro_val = nullptr, *ro_rew = nullptr, *ro_y = nullptr,
          *ro_adv = nullptr, *ro_boot = nullptr;
    // the gradient step's workspace over `chunk` env-samples
    int chunk = 0;
    FieldActs tw;
    float *dxl[FIELD_MAX_LAYERS + 1], *dzc = nullptr, *cslab = nullptr, *slab = nullptr;
    float *dd1 = nullptr, *dd2 = nullptr, *dp1 = nullptr, *dp2 = nullptr, *dv1 = nullptr, *dv2 = nullptr, *dzh = nullptr, *zvs = nullptr;
    int32_t *cell_count = nullptr, *cell_off = nullptr, *cell_list = nullptr;      // the chunk's agent-samples listed per grid cell
    FieldEval ev;                  // grl_fieldnet_eval's outputs (net_field_eval.inc)
};

// element (k, col) of a head matrix: base[k * sk + col * sc] -- row-major mu_w (sk = HWA, sc = 1) or the column-major copy (1, P2)
struct HeadView {
    const float *mu, *sg;
    long sk, sc;
};

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ void field_transpose_kernel(const float *__restrict__ src, long rows, long cols, float *__restrict__ dst) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const long c = i / rows, r = i - c * rows;
    dst[i] = src[r * cols + c];
}

// float32(count / 80.0), float32(count / 10.0): the reference divides float64 counts (state_processors.py:43-44)
__device__ __forceinline__ float field_density(int count, int channel) { return (float)((double)count / (channel ? 10.0 : 80.0)); }

// the (G, G, 2) images of n envs from their compact observations; one workgroup per env, integer counts first
__global__ __launch_bounds__(256) void field_grid_kernel(const uint8_t *__restrict__ lb, const uint8_t *__restrict__ ab, int G, float *__restrict__ out) {
    const long env = blockIdx.x;
    const int n = G * G * 2, tid = threadIdx.x;
    int *cnt = reinterpret_cast<int *>(out + env * n);
    for (int i = tid; i < n; i += 256) cnt[i] = 0;
    __syncthreads();
    if (tid < N_POINTS) {
        const uint8_t *b = tid < N_LOCUSTS ? lb + env * (N_LOCUSTS * 2) + tid * 2 : ab + env * (N_AGENTS * 2) + (tid - N_LOCUSTS) * 2;
        const int bx = b[0], by = b[1];
        if (bx < G && by < G) atomicAdd(&cnt[(bx * G + by) * 2 + (tid < N_LOCUSTS ? 0 : 1)], 1);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int c = cnt[i];
        out[env * n + i] = field_density(c, i & 1);
    }
}

// SwarmRunner.transform_actions_for_env (emulator_runner.py:113-118): transform_kernel's statements (rollout_math.hip)
__device__ __forceinline__ float2 field_norm_clip(float2 r) {
    const float d = sqrtf(r.x * r.x + r.y * r.y);
    if (d >= 1.0f) { r.x /= d; r.y /= d; }
    return r;
}

// a = mu + sigma * N(0,1) (paac.py:418) in float64, then the norm clip
__device__ __forceinline__ void field_sample_one(float2 m, float2 s, uint64_t seed, uint32_t env_id, uint32_t counter, uint32_t agent, float2 *raw,
                                                 float2 *envact) {
    double e0, e1;
    normal_pair(rng_block(seed, env_id, counter, RS_FIELD_ACTION, agent), e0, e1);
    const float2 r = make_float2((float)((double)m.x + (double)s.x * e0), (float)((double)m.y + (double)s.y * e1));
    *raw = r;
    *envact = field_norm_clip(r);
}

// what one env's forward reads besides its observation (field_env_forward)
struct FieldFwdArgs {
    const float *P;
    HeadView hv;
    FieldOff o;
    int G, F, L, P2, HWA, D0, m0n, m1n;
    float scale;
};

struct FieldStepArgs : FieldFwdArgs {
    const uint8_t *lb, *ab, *pos;      // the handle's observation
    int nenv;
    float *mu, *sigma, *vs;            // (B,2) (B,2) (B)
    float *raw, *envact;               // (B,2) each, or nullptr: no sampling, no record
    uint64_t seed;
    uint32_t env_off, counter;
    uint32_t *ro_lb, *ro_ab, *ro_pos;
    int32_t *done_count;
};

__device__ __forceinline__ void field_record_obs(const FieldStepArgs &a, int i, int stride) {
    const uint32_t *lb = reinterpret_cast<const uint32_t *>(a.lb), *ab = reinterpret_cast<const uint32_t *>(a.ab), *ps = reinterpret_cast<const uint32_t *>(a.pos);
    for (int w = i; w < a.nenv * 50; w += stride) {      // 40 + 5 + 5 words per env
        if (w < a.nenv * 40) a.ro_lb[w] = lb[w];
        else if (w < a.nenv * 45) a.ro_ab[w - a.nenv * 40] = ab[w - a.nenv * 40];
        else a.ro_pos[w - a.nenv * 45] = ps[w - a.nenv * 45];
    }
}

// U > 1: U rows' loads in flight per wait (the whole-episode kernel, whose compiler otherwise waits for every load); the sum's order stays
template <int U>
__device__ __forceinline__ void field_lds_dense(const float *in, const float *__restrict__ w, const float *__restrict__ b, int K, int J, float *out, int t0,
                                                int nt) {
    for (int j = t0; j < J; j += nt) {
        float acc = b[j];
        if (U > 1) {
#pragma unroll U
            for (int k = 0; k < K; ++k) acc += in[k] * w[(long)k * J + j];
        } else {
            for (int k = 0; k < K; ++k) acc += in[k] * w[(long)k * J + j];
        }
        out[j] = fmaxf(acc, 0.f);
    }
}

// floats of one env's forward in LDS: the image, the two pooled maps, d1 d2 p1 v1 v2, p2
static size_t field_fwd_floats(int G, int m0n, int m1n, int P2) { return (size_t)G * G * 2 + m0n + m1n + 64 + 32 + 64 + 64 + 32 + P2; }

// One env's forward out of LDS (field_fwd_floats) on the nt lanes of its workgroup (whole waves, at least two); sums in the order of
// field_conv_pool / field_dense / field_heads_fwd.  lb / ab / pos: the env's compact observation, in global memory or in LDS -- bytes
// written just before the call are ordered by the first barrier below.  emit(agent, mu, sigma, vs) runs on lane 0 of the agent's
// wave; no barrier follows it.  Every output element is one lane's sequential sum and the head sums are 64-lane field_wave_sums,
// so nt decides which lane computes an element, not its bits (field_fused_step_kernel: 256 lanes, field_eval_kernel: 320).
template <int U = 0, typename EMIT>
__device__ __forceinline__ void field_env_forward(const FieldFwdArgs &a, const uint8_t *lb, const uint8_t *ab, const uint8_t *pos, float *lds, int tid,
                                                  int nt, EMIT &&emit) {
    const int G = a.G, n0 = G * G * 2;
    float *img = lds, *m0 = img + n0, *m1 = m0 + a.m0n, *d1 = m1 + a.m1n, *d2 = d1 + 64, *p1 = d2 + 32, *v1 = p1 + 64, *v2 = v1 + 64, *p2 = v2 + 32;
    int *cnt = reinterpret_cast<int *>(img);
    for (int i = tid; i < n0; i += nt) cnt[i] = 0;
    __syncthreads();
    if (tid < N_POINTS) {
        const uint8_t *b = tid < N_LOCUSTS ? lb + tid * 2 : ab + (tid - N_LOCUSTS) * 2;
        const int bx = b[0], by = b[1];
        if (bx < G && by < G) atomicAdd(&cnt[(bx * G + by) * 2 + (tid < N_LOCUSTS ? 0 : 1)], 1);
    }
    __syncthreads();
    for (int i = tid; i < n0; i += nt) {
        const int c = cnt[i];
        img[i] = field_density(c, i & 1);
    }
    __syncthreads();
    const float *in = img;
    int H = G, Cin = 2;
    for (int l = 0; l < a.L; ++l) {
        float *out = (l & 1) ? m1 : m0;
        const float *w = a.P + a.o.cw[l], *b = a.P + a.o.cb[l];
        const int F = a.F, H2 = H / 2, total = H2 * H2 * F;
        for (int i = tid; i < total; i += nt) {
            const int f = i % F, x2 = (i / F) % H2, y2 = i / (F * H2);
            float best = 0.f;
            for (int d = 0; d < 4; ++d) {
                const int yy = 2 * y2 + (d >> 1), xx = 2 * x2 + (d & 1);
                float acc = b[f];
                for (int ky = 0; ky < 3; ++ky) {
                    const int iy = yy + ky - 1;
                    if ((unsigned)iy >= (unsigned)H) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ix = xx + kx - 1;
                        if ((unsigned)ix >= (unsigned)H) continue;
                        const float *xp = in + (iy * H + ix) * Cin;
                        const float *wp = w + (long)((ky * 3 + kx) * Cin) * F + f;
                        for (int ci = 0; ci < Cin; ++ci) acc += xp[ci] * wp[(long)ci * F];
                    }
                }
                const float v = fmaxf(acc, 0.f);
                if (d == 0 || v > best) best = v;
            }
            out[i] = best;
        }
        __syncthreads();
        in = out; H = H2; Cin = F;
    }
    const FieldOff &o = a.o;
    field_lds_dense<U>(in, a.P + o.d1w, a.P + o.d1b, a.D0, 64, d1, tid, nt);
    __syncthreads();
    field_lds_dense<U>(d1, a.P + o.d2w, a.P + o.d2b, 64, 32, d2, tid, nt);
    __syncthreads();
    const int half = nt / 2;      // the two towers side by side: 128 + 128 lanes of 256, 160 + 160 of 320
    if (tid < half) field_lds_dense<U>(d2, a.P + o.p1w, a.P + o.p1b, 32, 64, p1, tid, half);
    else field_lds_dense<U>(d2, a.P + o.v1w, a.P + o.v1b, 32, 64, v1, tid - half, nt - half);
    __syncthreads();
    field_lds_dense<U>(p1, a.P + o.p2w, a.P + o.p2b, 64, a.P2, p2, tid, nt);
    field_lds_dense<U>(v1, a.P + o.v2w, a.P + o.v2b, 64, 32, v2, tid, nt);
    __syncthreads();
    // the ten agents: a wave per agent, lanes over the rows of its 2A columns
    const int wave = tid >> 6, lane = tid & 63, waves = nt >> 6;
    float zv = lane < FIELD_FC ? v2[lane] * a.P[o.v3w + lane] : 0.f;
    zv = field_wave_sum(zv) + a.P[o.v3b];
    const float vs = -a.scale * (zv > 20.f ? zv : log1pf(expf(zv)));
    for (int ag = wave; ag < FR_AGENTS; ag += waves) {
        const uint8_t *pp = pos + ag * 2;
        const int px = min((int)pp[0], G - 1), py = min((int)pp[1], G - 1);
        const long col = (long)(px * G + py) * FR_A;
        const float *mw = a.hv.mu + col * a.hv.sc, *sw = a.hv.sg + col * a.hv.sc;
        float mx = 0.f, my = 0.f, sx = 0.f, sy = 0.f;
        for (int k = lane; k < a.P2; k += 64) {
            const float xv = p2[k];
            const long r = (long)k * a.hv.sk;
            mx += xv * mw[r]; sx += xv * sw[r];
            my += xv * mw[r + a.hv.sc]; sy += xv * sw[r + a.hv.sc];
        }
        mx = field_wave_sum(mx); sx = field_wave_sum(sx); my = field_wave_sum(my); sy = field_wave_sum(sy);
        if (lane == 0) {
            const float2 m = make_float2(tanhf(mx + a.P[o.mub + col]), tanhf(my + a.P[o.mub + col + 1]));
            const float2 s = make_float2(1.0f / (1.0f + expf(-(sx + a.P[o.sgb + col]))), 1.0f / (1.0f + expf(-(sy + a.P[o.sgb + col + 1]))));
            emit(ag, m, s, vs);
        }
    }
}

// One step's forward of one env per workgroup, from the handle's observation in global memory.
__global__ __launch_bounds__(256) void field_fused_step_kernel(FieldStepArgs a) {
    extern __shared__ float lds[];
    const int env = blockIdx.x, tid = threadIdx.x;
    if (a.raw) {
        if (env == 0 && tid == 0 && a.done_count) *a.done_count = 0;      // the env step that follows on this stream appends to it
        field_record_obs(a, env * 256 + tid, gridDim.x * 256);
    }
    field_env_forward(a, a.lb + (long)env * (N_LOCUSTS * 2), a.ab + (long)env * (N_AGENTS * 2), a.pos + (long)env * (N_AGENTS * 2), lds, tid, 256,
                      [&](int ag, float2 m, float2 s, float vs) {
                          const long i = (long)env * FR_AGENTS + ag;
                          reinterpret_cast<float2 *>(a.mu)[i] = m;
                          reinterpret_cast<float2 *>(a.sigma)[i] = s;
                          a.vs[i] = vs;
                          if (a.raw) field_sample_one(m, s, a.seed, (uint32_t)env + a.env_off, a.counter, (uint32_t)ag, reinterpret_cast<float2 *>(a.raw) + i,
                                                      reinterpret_cast<float2 *>(a.envact) + i);
                      });
}

// the heads of agent-samples [0, n) of a chunk whose env-rows are in p2 / v2: sample i reads row i / 10.  One wave per sample,
// the sums of field_heads_fwd_kernel.  pos: the chunk's (envs,10,2) bytes; outputs at the chunk's first sample.
__global__ __launch_bounds__(256) void field_heads_env_kernel(const float *__restrict__ p2, const float *__restrict__ v2, const uint8_t *__restrict__ pos,
                                                              const float *__restrict__ P, HeadView hv, FieldOff o, int n, int P2, int G, float scale,
                                                              float *__restrict__ mu, float *__restrict__ sigma, float *__restrict__ vs) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int row = i / FR_AGENTS;
    const int px = min((int)pos[i * 2], G - 1), py = min((int)pos[i * 2 + 1], G - 1);
    const long col = (long)(px * G + py) * FR_A;
    const float *mw = hv.mu + col * hv.sc, *sw = hv.sg + col * hv.sc;
    float m[FR_A] = {0.f, 0.f}, s[FR_A] = {0.f, 0.f}, zv = 0.f;
    for (int k = lane; k < P2; k += 64) {
        const float xv = p2[(long)row * P2 + k];
#pragma unroll
        for (int a = 0; a < FR_A; ++a) { m[a] += xv * mw[(long)k * hv.sk + a * hv.sc]; s[a] += xv * sw[(long)k * hv.sk + a * hv.sc]; }
    }
    if (lane < FIELD_FC) zv = v2[(long)row * FIELD_FC + lane] * P[o.v3w + lane];
#pragma unroll
    for (int a = 0; a < FR_A; ++a) { m[a] = field_wave_sum(m[a]); s[a] = field_wave_sum(s[a]); }
    zv = field_wave_sum(zv);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < FR_A; ++a) {
            mu[(long)i * FR_A + a] = tanhf(m[a] + P[o.mub + col + a]);
            sigma[(long)i * FR_A + a] = 1.0f / (1.0f + expf(-(s[a] + P[o.sgb + col + a])));
        }
        zv += P[o.v3b];
        vs[i] = -scale * (zv > 20.f ? zv : log1pf(expf(zv)));
    }
}

// the layer-by-layer step's sampling, norm clip and observation record (sample_actions_kernel of the conv rollout)
__global__ void field_sample_kernel(FieldStepArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && a.done_count) *a.done_count = 0;
    field_record_obs(a, i, gridDim.x * blockDim.x);
    if (i >= a.nenv * FR_AGENTS) return;
    const int env = i / FR_AGENTS, ag = i - env * FR_AGENTS;
    field_sample_one(reinterpret_cast<const float2 *>(a.mu)[i], reinterpret_cast<const float2 *>(a.sigma)[i], a.seed, (uint32_t)env + a.env_off, a.counter,
                     (uint32_t)ag, reinterpret_cast<float2 *>(a.raw) + i, reinterpret_cast<float2 *>(a.envact) + i);
}

__global__ void field_reward_layout_kernel(const float *__restrict__ reward, int ne, int layout, float *__restrict__ out, const uint8_t *__restrict__ done,
                                           uint8_t *__restrict__ ro_done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ne) ro_done[i] = done[i];
    if (layout == 0) {
        if (i < ne * FR_AGENTS) out[i] = reward[i / FR_AGENTS];
    } else if (i < ne) {
        out[i] = reward[i];      // quirk Q4: the reference's (E,) rewards land in the first E of the B columns
    }
}

// ---- the gradient step.  Env-sample es of a chunk owns agent-samples es * 10 .. es * 10 + 9 (pointers at the chunk's first).
// Loss terms and dZ of the heads per agent-sample (the dzh row of field_heads_bwd_kernel), then for the shared trunk
//   dp2[es] = relu'(p2) . sum_agents (mu_w[:, cols] dz_mu + sigma_w[:, cols] dz_sigma),  zvs[es] = sum_agents dz_v,
//   dv2[es] = relu'(v2) . v3_w zvs  -- agents in order.  One wave per env-sample; every lane holds the ten agents' dZ.
__global__ __launch_bounds__(256) void fr_heads_bwd_kernel(const float *__restrict__ p2, const float *__restrict__ v2, const uint8_t *__restrict__ pos,
                                                           const float *__restrict__ mu, const float *__restrict__ sigma, const float *__restrict__ vs,
                                                           const float *__restrict__ actions, const float *__restrict__ adv, const float *__restrict__ y,
                                                           const float *__restrict__ P, HeadView hv, FieldOff o, int n, int P2, int G, float scale,
                                                           float beta, float inv_n, float *__restrict__ dzh, float *__restrict__ dp2,
                                                           float *__restrict__ dv2, float *__restrict__ zvs) {
    const int es = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (es >= n) return;
    float zm[FR_AGENTS][FR_A], zs[FR_AGENTS][FR_A], zsum = 0.f;
    long col[FR_AGENTS];
#pragma unroll
    for (int ag = 0; ag < FR_AGENTS; ++ag) {
        const long i = (long)es * FR_AGENTS + ag;
        const float Adv = adv[i], v = vs[i], tgt = y[i];
        const float dlogp = -Adv * inv_n, dent = -beta * inv_n;
        float logp = 0.f, ent = 0.f;
#pragma unroll
        for (int a = 0; a < FR_A; ++a) {
            const float m = mu[i * FR_A + a], s = sigma[i * FR_A + a], d = actions[i * FR_A + a] - m;
            logp += -0.5f * (d / s) * (d / s) - logf(s) - 0.5f * FIELD_LOG_2PI;
            ent += 0.5f + 0.5f * FIELD_LOG_2PI + logf(s);
            const float dmu = dlogp * d / (s * s);
            const float dsg = dlogp * (d * d / (s * s * s) - 1.0f / s) + dent / s;
            zm[ag][a] = dmu * (1.0f - m * m);
            zs[ag][a] = dsg * s * (1.0f - s);
        }
        const float dvs = 0.5f * (v - tgt) / scale * inv_n;
        const float zv = dvs * (-scale) * (-expm1f(v / scale));
        zsum += zv;
        if (lane == 0) {
            float *q = dzh + i * FR_DZ;
#pragma unroll
            for (int a = 0; a < FR_A; ++a) { q[a] = zm[ag][a]; q[FR_A + a] = zs[ag][a]; }
            q[2 * FR_A] = zv;
            q[2 * FR_A + 1] = -(logp * Adv + beta * ent);
            q[2 * FR_A + 2] = 0.25f * (v - tgt) * (v - tgt) / scale;
        }
        const int px = min((int)pos[i * 2], G - 1), py = min((int)pos[i * 2 + 1], G - 1);
        col[ag] = (long)(px * G + py) * FR_A;
    }
    for (int k = lane; k < P2; k += 64) {
        const long r = (long)k * hv.sk;
        float g = 0.f;
#pragma unroll
        for (int ag = 0; ag < FR_AGENTS; ++ag) {
            const float *mw = hv.mu + col[ag] * hv.sc + r, *sw = hv.sg + col[ag] * hv.sc + r;
            float ga = 0.f;
#pragma unroll
            for (int a = 0; a < FR_A; ++a) ga += zm[ag][a] * mw[a * hv.sc];
#pragma unroll
            for (int a = 0; a < FR_A; ++a) ga += zs[ag][a] * sw[a * hv.sc];
            g += ga;
        }
        dp2[(long)es * P2 + k] = p2[(long)es * P2 + k] > 0.f ? g : 0.f;
    }
    if (lane < FIELD_FC) dv2[(long)es * FIELD_FC + lane] = v2[(long)es * FIELD_FC + lane] > 0.f ? zsum * P[o.v3w + lane] : 0.f;
    if (lane == 0) zvs[es] = zsum;
}

// Head weight gradients.  Agents that share a cell -- within an env, across envs and steps -- add into the same columns of mu_w /
// sigma_w, so the chunk's agent-samples are first listed per cell in (t, env, agent) order: fr_cell_scan (one wave per cell, 64
// positions per ballot) counts a cell's visitors, fr_cell_offsets turns the counts into offsets, a second fr_cell_scan writes the
// visitors behind the cell's offset.  fr_heads_wgrad then walks a cell's list in order, one wave per 64 rows, eight visitors'
// loads in flight at a time (a hot cell is a long chain of dependent adds, not of dependent loads).  Chunks follow each other on
// the stream; G was zeroed before the first.
__global__ __launch_bounds__(64) void fr_cell_scan_kernel(const uint8_t *__restrict__ pos, long nag, int G, const int32_t *__restrict__ offsets,
                                                          int32_t *__restrict__ counts, int32_t *__restrict__ list) {
    const int cell = blockIdx.x, lane = threadIdx.x;
    int n = 0;
    const int at = offsets ? offsets[cell] : 0;
    for (long base = 0; base < nag; base += 64) {
        const long i = base + lane;
        bool match = false;
        if (i < nag) match = min((int)pos[i * 2], G - 1) * G + min((int)pos[i * 2 + 1], G - 1) == cell;
        const unsigned long long mask = __ballot(match);
        if (offsets && match) list[at + n + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)i;
        n += __popcll(mask);
    }
    if (!offsets && lane == 0) counts[cell] = n;
}

__global__ void fr_cell_offsets_kernel(const int32_t *__restrict__ counts, int cells, int32_t *__restrict__ offsets) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int at = 0;
    for (int c = 0; c < cells; ++c) { offsets[c] = at; at += counts[c]; }
}

__global__ __launch_bounds__(64) void fr_heads_wgrad_kernel(const float *__restrict__ p2, const float *__restrict__ dzh, const int32_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ counts, const int32_t *__restrict__ list, FieldOff o, int P2,
                                                            int HWA, float *__restrict__ Gr) {
    const int cell = blockIdx.x, lane = threadIdx.x, k = blockIdx.y * 64 + lane, n = counts[cell];
    if (n == 0) return;
    const int32_t *mine = list + offsets[cell];
    const bool row = k < P2;
    float am[FR_A] = {0.f, 0.f}, as[FR_A] = {0.f, 0.f}, bm[FR_A] = {0.f, 0.f}, bs[FR_A] = {0.f, 0.f};
    constexpr int U = 8;
    for (int i0 = 0; i0 < n; i0 += U) {
        float pv[U], q[U][2 * FR_A];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = i0 + u < n;
            const long ii = on ? mine[i0 + u] : 0;
            pv[u] = on && row ? p2[(ii / FR_AGENTS) * P2 + k] : 0.f;
#pragma unroll
            for (int a = 0; a < 2 * FR_A; ++a) q[u][a] = on ? dzh[ii * FR_DZ + a] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i0 + u >= n) break;
#pragma unroll
            for (int a = 0; a < FR_A; ++a) { am[a] += pv[u] * q[u][a]; as[a] += pv[u] * q[u][FR_A + a]; bm[a] += q[u][a]; bs[a] += q[u][FR_A + a]; }
        }
    }
    const long col = (long)cell * FR_A;
    if (row) {
#pragma unroll
        for (int a = 0; a < FR_A; ++a) {
            Gr[o.muw + (long)k * HWA + col + a] += am[a];
            Gr[o.sgw + (long)k * HWA + col + a] += as[a];
        }
    }
    if (blockIdx.y == 0 && lane < FR_A) {
        Gr[o.mub + col + lane] += bm[lane];
        Gr[o.sgb + col + lane] += bs[lane];
    }
}

// the chunk's policy and critic terms added to stats64[0..1] in float64: strided partial sums, a tree inside the one block
__global__ __launch_bounds__(256) void fr_loss_sum_kernel(const float *__restrict__ dzh, long nag, double *__restrict__ stats64) {
    __shared__ double red[2][256];
    double s0 = 0.0, s1 = 0.0;
    for (long i = threadIdx.x; i < nag; i += 256) { s0 += (double)dzh[i * FR_DZ + 2 * FR_A + 1]; s1 += (double)dzh[i * FR_DZ + 2 * FR_A + 2]; }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { red[0][threadIdx.x] += red[0][threadIdx.x + w]; red[1][threadIdx.x] += red[1][threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { stats64[0] += red[0][0]; stats64[1] += red[1][0]; }
}

// slab[s][k][j] = sum over the samples n of split s (in order) of in[n][k] dout[n][j]; row k == K is the bias (in = 1).
// grid (J / 256, (K + 1) / FR_KT, splits): a lane owns FR_KT rows of one column, so dout is read once per FR_KT rows.
__global__ __launch_bounds__(256) void fr_dense_wgrad_kernel(const float *__restrict__ in, const float *__restrict__ dout, long N, int K, int J,
                                                             float *__restrict__ slab) {
    const int j = blockIdx.x * 256 + threadIdx.x, k0 = blockIdx.y * FR_KT;
    if (j >= J) return;
    const long n0 = (long)blockIdx.z * FR_SPLIT, n1 = n0 + FR_SPLIT < N ? n0 + FR_SPLIT : N;
    float acc[FR_KT];
#pragma unroll
    for (int kk = 0; kk < FR_KT; ++kk) acc[kk] = 0.f;
    for (long n = n0; n < n1; ++n) {
        const float dv = dout[n * J + j];
#pragma unroll
        for (int kk = 0; kk < FR_KT; ++kk) {
            const int k = k0 + kk;
            if (k < K) acc[kk] += in[n * K + k] * dv;
            else if (k == K) acc[kk] += dv;
        }
    }
    float *sl = slab + (long)blockIdx.z * (K + 1) * J;
#pragma unroll
    for (int kk = 0; kk < FR_KT; ++kk)
        if (k0 + kk <= K) sl[(long)(k0 + kk) * J + j] = acc[kk];
}

// din[n][k] = relu'(fwd[n][k]) . sum_j dout[n][j] W[k][j] for the 64 rows of pol2's input: 32 samples x 64 rows per workgroup, dout
// and W through LDS in tiles of 32 columns (field_dense_dgrad_kernel gives a lane one row of W to stream: 64 cache lines per load).
// j ascends per output, so the bits are that kernel's.
__global__ __launch_bounds__(256) void fr_dgrad64_kernel(const float *__restrict__ dout, const float *__restrict__ w, const float *__restrict__ fwd, long N,
                                                         int J, float *__restrict__ din) {
    __shared__ float A[32][33], B[64][33];
    const int tid = threadIdx.x, kk = tid & 63, ng = tid >> 6;
    const long n0 = (long)blockIdx.x * 32;
    float acc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[s] = 0.f;
    for (int j0 = 0; j0 < J; j0 += 32) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, s = e >> 5, jj = e & 31;
            A[s][jj] = (n0 + s < N && j0 + jj < J) ? dout[(n0 + s) * J + j0 + jj] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, k = e >> 5, jj = e & 31;
            B[k][jj] = j0 + jj < J ? w[(long)k * J + j0 + jj] : 0.f;
        }
        __syncthreads();
        const int jn = J - j0 < 32 ? J - j0 : 32;
        for (int jj = 0; jj < jn; ++jj) {
            const float b = B[kk][jj];
#pragma unroll
            for (int s = 0; s < 8; ++s) acc[s] += A[ng * 8 + s][jj] * b;
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const long n = n0 + ng * 8 + s;
        if (n < N) din[n * 64 + kk] = fwd[n * 64 + kk] > 0.f ? acc[s] : 0.f;
    }
}

// dst[s][i] = sum over rows r of split s (in order) of src[r][i]
__global__ void fr_rows_partial_kernel(const float *__restrict__ src, long rows, int width, float *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width) return;
    const long r0 = (long)blockIdx.y * FR_SPLIT, r1 = r0 + FR_SPLIT < rows ? r0 + FR_SPLIT : rows;
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += src[r * width + i];
    dst[(long)blockIdx.y * width + i] = s;
}

// g[i] += slab[0][i] + slab[1][i] + ... (in order)
__global__ void fr_accum_kernel(const float *__restrict__ slab, int splits, int width, float *__restrict__ g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width) return;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += slab[(long)k * width + i];
    g[i] += s;
}

// ---------------------------------------------------------------------------------------------------------------- host side
static int fr_check(grl_fieldnet *net, const char *fn) {
    const grl_handle *h = net->h;
    const grl_fieldnet_config &c = net->cfg;
    if (h->cfg.env_kind != GRL_ENV_SWARM) return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": the net is not on a Swarm handle");
    if (c.height != c.width || c.height != h->cfg.grid_size)
        return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": the handle's grid_size " + std::to_string(h->cfg.grid_size) + " is not the net's " +
                                                 std::to_string(c.height) + "x" + std::to_string(c.width) + " field");
    if (c.channels != 2) return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": the Swarm density image has 2 channels; this net was built with " + std::to_string(c.channels));
    if (c.num_actions != FR_A) return paac_fail(net, GRL_E_INVALID, std::string(fn) + ": SwarmEnv.step takes (10, 2) actions; this net was built with num_actions != 2");
    return GRL_OK;
}

static HeadView fr_head_view(const grl_fieldnet *net) {
    const FieldRollout *r = net->ro;
    if (r->headt) return HeadView{r->muwt, r->sgwt, 1, (long)net->P2};
    return HeadView{net->params + net->off.muw, net->params + net->off.sgw, (long)net->HWA, 1};
}

// first use: the environment switches, the per-batch buffers; every use: the column-major head copies follow the parameters
static int fr_prepare(grl_fieldnet *net, const char *fn) {
    int rc = fr_check(net, fn);
    if (rc) return rc;
    hipSetDevice(net->h->cfg.device_id);
    if (!net->ro) net->ro = new FieldRollout();
    FieldRollout *r = net->ro;
    hipStream_t st = net->h->stream;
    if (r->fused < 0) {
        const char *ev = getenv("GRL_FIELD_FUSED");
        const char *ht = getenv("GRL_FIELD_HEADT");
        r->headt = !(ht && std::string(ht) == "off");
        const int G = net->cfg.height;
        r->m0n = (G / 2) * (G / 2) * net->F;
        r->m1n = net->L >= 2 ? (G / 4) * (G / 4) * net->F : 0;
        r->lds_bytes = field_fwd_floats(G, r->m0n, r->m1n, net->P2) * sizeof(float);
        const size_t B = (size_t)net->h->E * FR_AGENTS;
        if ((rc = paac_alloc(net, &r->cur_mu, B * FR_A)) || (rc = paac_alloc(net, &r->cur_sg, B * FR_A)) || (rc = paac_alloc(net, &r->cur_vs, B))) return rc;
        if (r->headt && ((rc = paac_alloc(net, &r->muwt, (size_t)net->P2 * net->HWA)) || (rc = paac_alloc(net, &r->sgwt, (size_t)net->P2 * net->HWA)))) return rc;
        int fused = !(ev && std::string(ev) == "off") && r->lds_bytes <= FR_LDS_BYTES;
        if (fused && r->lds_bytes > 48 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(field_fused_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r->lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            fused = 0;
        }
        r->fused = fused;
    }
    if (r->headt && r->headt_version != net->param_version) {
        const long n = (long)net->P2 * net->HWA;
        hipLaunchKernelGGL(field_transpose_kernel, dim3(nb(n)), dim3(256), 0, st, net->params + net->off.muw, (long)net->P2, (long)net->HWA, r->muwt);
        hipLaunchKernelGGL(field_transpose_kernel, dim3(nb(n)), dim3(256), 0, st, net->params + net->off.sgw, (long)net->P2, (long)net->HWA, r->sgwt);
        PAAC_HIP(net, hipGetLastError());
        r->headt_version = net->param_version;
    }
    return GRL_OK;
}

// forward on the handle's current observation; a.raw != nullptr: sample, clip and record as well
static int fr_forward_current(grl_fieldnet *net, FieldStepArgs a) {
    grl_handle *h = net->h;
    FieldRollout *r = net->ro;
    hipStream_t st = h->stream;
    const int E = h->E, G = net->cfg.height;
    a.lb = h->sw.lbins; a.ab = h->sw.abins; a.pos = h->sw.pos;
    a.P = net->params; a.hv = fr_head_view(net); a.o = net->off;
    a.G = G; a.F = net->F; a.L = net->L; a.P2 = net->P2; a.HWA = net->HWA; a.D0 = net->D0; a.m0n = r->m0n; a.m1n = r->m1n; a.nenv = E;
    a.scale = net->cfg.scale;
    a.seed = h->cfg.seed; a.env_off = (uint32_t)h->cfg.env_id_offset;
    a.done_count = h->done_count;
    if (r->fused) {
        hipLaunchKernelGGL(field_fused_step_kernel, dim3(E), dim3(256), r->lds_bytes, st, a);
    } else {
        const FieldActs acts = field_net_acts(net);
        const int ms = net->cfg.max_samples;
        for (int e0 = 0; e0 < E; e0 += ms) {
            const int ne = E - e0 < ms ? E - e0 : ms;
            hipLaunchKernelGGL(field_grid_kernel, dim3(ne), dim3(256), 0, st, a.lb + (size_t)e0 * 160, a.ab + (size_t)e0 * 20, G, acts.x[0]);
            field_trunk(net, acts, ne);
            hipLaunchKernelGGL(field_heads_env_kernel, dim3((ne * FR_AGENTS + 3) / 4), dim3(256), 0, st, acts.p2, acts.v2, a.pos + (size_t)e0 * 20, a.P, a.hv,
                               a.o, ne * FR_AGENTS, a.P2, G, a.scale, a.mu + (size_t)e0 * FR_AGENTS * FR_A, a.sigma + (size_t)e0 * FR_AGENTS * FR_A,
                               a.vs + (size_t)e0 * FR_AGENTS);
        }
        if (a.raw) hipLaunchKernelGGL(field_sample_kernel, dim3((E * FR_AGENTS + 255) / 256), dim3(256), 0, st, a);
    }
    PAAC_HIP(net, hipGetLastError());
    return GRL_OK;
}

static int fr_ensure_rollout_bufs(grl_fieldnet *net, int T) {
    FieldRollout *r = net->ro;
    if (r->ro_lb && r->cap_T >= T) return GRL_OK;
    const size_t E = net->h->E, B = E * FR_AGENTS, t = T;
    int rc;
    if ((rc = paac_alloc(net, &r->ro_lb, t * E * 160)) || (rc = paac_alloc(net, &r->ro_ab, t * E * 20)) || (rc = paac_alloc(net, &r->ro_pos, t * E * 20)) ||
        (rc = paac_alloc(net, &r->ro_done, t * E)) || (rc = paac_alloc(net, &r->ro_act, t * B * FR_A)) || (rc = paac_alloc(net, &r->ro_envact, t * B * FR_A)) ||
        (rc = paac_alloc(net, &r->ro_mu, t * B * FR_A)) || (rc = paac_alloc(net, &r->ro_sg, t * B * FR_A)) || (rc = paac_alloc(net, &r->ro_val, t * B)) ||
        (rc = paac_alloc(net, &r->ro_rew, t * B)) || (rc = paac_alloc(net, &r->ro_y, t * B)) || (rc = paac_alloc(net, &r->ro_adv, t * B)) ||
        (rc = paac_alloc(net, &r->ro_boot, B)))
        return rc;
    r->cap_T = T;
    r->chunk = 0;      // the gradient step sizes its workspace by (T, E)
    return GRL_OK;
}

// floats of the gradient step's workspace per env-sample
static size_t fr_ws_floats(const grl_fieldnet *net) {
    size_t f = 0, maxconv = 0, maxT = 0;
    for (int l = 0; l <= net->L; ++l) {
        const size_t e = (size_t)net->lh[l] * net->lw[l] * net->lc[l];
        f += e;
        if (l >= 1) f += e + (e + 3) / 4;
        if (l < net->L) {
            maxconv = std::max(maxconv, (size_t)net->lh[l] * net->lw[l] * net->F);
            maxT = std::max(maxT, 9 * (size_t)net->lc[l] * net->F + net->F);
        }
    }
    return f + maxconv + maxT + 2 * (64 + 32 + 64 + 64 + 32 + (size_t)net->P2) + FR_AGENTS * FR_DZ + 1;
}

static int fr_ensure_train_ws(grl_fieldnet *net) {
    FieldRollout *r = net->ro;
    // chunk: at most 8192 env-samples and ~256 MB of workspace, whole slabs -- a matter of the geometry alone; the workspace is not
    // larger than the rollout buffers, which changes nothing for a rollout that fits one chunk, so the order of every sum is
    // fixed by (T, E, geometry)
    long chunk = (long)(((size_t)256 << 20) / (fr_ws_floats(net) * sizeof(float)));
    chunk = std::max<long>(FR_SPLIT, std::min<long>(8192, chunk / FR_SPLIT * FR_SPLIT));
    const long cap = (long)r->cap_T * net->h->E;
    if (chunk > cap) chunk = cap;
    if (r->chunk == chunk) return GRL_OK;
    const size_t c = (size_t)chunk;
    int rc = GRL_OK;
    auto Al = [&](float **q, size_t cnt) { if (rc == GRL_OK) rc = paac_alloc(net, q, cnt); };
    size_t maxconv = 0, maxT = 0;
    for (int l = 0; l <= net->L; ++l) {
        const size_t e = c * net->lh[l] * net->lw[l] * net->lc[l];
        Al(&r->tw.x[l], e);
        r->dxl[l] = nullptr;
        if (l >= 1) { Al(&r->dxl[l], e); if (rc == GRL_OK) rc = paac_alloc(net, &r->tw.idx[l - 1], e); }
        if (l < net->L) {
            maxconv = std::max(maxconv, c * net->lh[l] * net->lw[l] * net->F);
            maxT = std::max(maxT, 9 * (size_t)net->lc[l] * net->F + net->F);
        }
    }
    Al(&r->dzc, maxconv); Al(&r->cslab, c * maxT);
    Al(&r->tw.d1, c * 64); Al(&r->tw.d2, c * 32); Al(&r->tw.p1, c * 64); Al(&r->tw.p2, c * net->P2); Al(&r->tw.v1, c * 64); Al(&r->tw.v2, c * 32);
    Al(&r->dd1, c * 64); Al(&r->dd2, c * 32); Al(&r->dp1, c * 64); Al(&r->dp2, c * net->P2); Al(&r->dv1, c * 64); Al(&r->dv2, c * 32);
    Al(&r->dzh, c * FR_AGENTS * FR_DZ); Al(&r->zvs, c);
    const size_t cells = (size_t)net->cfg.height * net->cfg.width;
    if (rc == GRL_OK) rc = paac_alloc(net, &r->cell_count, cells);
    if (rc == GRL_OK) rc = paac_alloc(net, &r->cell_off, cells);
    if (rc == GRL_OK) rc = paac_alloc(net, &r->cell_list, c * FR_AGENTS);
    const size_t splits = (c + FR_SPLIT - 1) / FR_SPLIT;
    const size_t width = std::max(std::max((size_t)(2 * FIELD_FC + 1) * net->P2, (size_t)(net->D0 + 1) * 2 * FIELD_FC), maxT);
    Al(&r->slab, splits * width);
    if (rc == GRL_OK) r->chunk = (int)chunk;
    return rc;
}

static int fr_train(grl_fieldnet *net, float lr, float *stats_host, int finish) {
    const char *fn = finish ? "grl_fieldnet_train_rollout" : "grl_fieldnet_train_rollout_grads";
    if (!net) return GRL_E_INVALID;
    if (!net->ro || net->ro->T <= 0) return paac_fail(net, GRL_E_STATE, std::string(fn) + ": no rollout to train on");
    int rc = fr_prepare(net, fn);
    if (rc) return rc;
    FieldRollout *r = net->ro;
    grl_handle *h = net->h;
    hipStream_t st = h->stream;
    const int E = h->E, T = r->T, G = net->cfg.height, P2 = net->P2, HWA = net->HWA;
    const long N = (long)T * E;
    if ((rc = fr_ensure_train_ws(net))) return rc;
    const float inv_n = 1.0f / ((float)T * (float)(E * FR_AGENTS));
    const float *P = net->params;
    float *Gr = net->grads;
    const FieldOff &o = net->off;
    const HeadView hv = fr_head_view(net);
    const FieldActs &tw = r->tw;
    PAAC_HIP(net, hipMemsetAsync(Gr, 0, (size_t)o.total * 4, st));
    PAAC_HIP(net, hipMemsetAsync(net->stats64, 0, 2 * sizeof(double), st));
    for (long c0 = 0; c0 < N; c0 += r->chunk) {
        const long n = N - c0 < r->chunk ? N - c0 : r->chunk, nag = n * FR_AGENTS, s0 = c0 * FR_AGENTS;
        const int splits = (int)((n + FR_SPLIT - 1) / FR_SPLIT);
        const uint8_t *pos = r->ro_pos + (size_t)c0 * 20;
        // same parameters as during the rollout: its mu / sigma / values are the gradient step's; the trunk is recomputed
        hipLaunchKernelGGL(field_grid_kernel, dim3((unsigned)n), dim3(256), 0, st, r->ro_lb + (size_t)c0 * 160, r->ro_ab + (size_t)c0 * 20, G, tw.x[0]);
        field_trunk(net, tw, (int)n);
        hipLaunchKernelGGL(fr_heads_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, tw.p2, tw.v2, pos, r->ro_mu + s0 * FR_A, r->ro_sg + s0 * FR_A,
                           r->ro_val + s0, r->ro_act + s0 * FR_A, r->ro_adv + s0, r->ro_y + s0, P, hv, o, (int)n, P2, G, net->cfg.scale, net->cfg.entropy_beta,
                           inv_n, r->dzh, r->dp2, r->dv2, r->zvs);
        hipLaunchKernelGGL(fr_cell_scan_kernel, dim3(G * G), dim3(64), 0, st, pos, nag, G, (const int32_t *)nullptr, r->cell_count, (int32_t *)nullptr);
        hipLaunchKernelGGL(fr_cell_offsets_kernel, dim3(1), dim3(64), 0, st, r->cell_count, G * G, r->cell_off);
        hipLaunchKernelGGL(fr_cell_scan_kernel, dim3(G * G), dim3(64), 0, st, pos, nag, G, r->cell_off, r->cell_count, r->cell_list);
        hipLaunchKernelGGL(fr_heads_wgrad_kernel, dim3(G * G, (P2 + 63) / 64), dim3(64), 0, st, tw.p2, r->dzh, r->cell_off, r->cell_count, r->cell_list, o, P2,
                           HWA, Gr);
        hipLaunchKernelGGL(fr_loss_sum_kernel, dim3(1), dim3(256), 0, st, r->dzh, nag, net->stats64);
        auto wgrad = [&](const float *in, const float *dout, int K, int J, long w) {      // the bias follows its matrix in the flat vector
            hipLaunchKernelGGL(fr_dense_wgrad_kernel, dim3((J + 255) / 256, (K + 1 + FR_KT - 1) / FR_KT, splits), dim3(256), 0, st, in, dout, n, K, J, r->slab);
            hipLaunchKernelGGL(fr_accum_kernel, dim3(nb((long)(K + 1) * J)), dim3(256), 0, st, r->slab, splits, (K + 1) * J, Gr + w);
        };
        auto dgrad = [&](const float *dout, long w, const float *fwd, int K, int J, int acc, float *din) {
            hipLaunchKernelGGL(field_dense_dgrad_kernel, dim3(nb(n * K)), dim3(256), 0, st, dout, P + w, fwd, n, K, J, acc, din);
        };
        wgrad(tw.v2, r->zvs, FIELD_FC, 1, o.v3w);
        wgrad(tw.p1, r->dp2, 2 * FIELD_FC, P2, o.p2w);
        static_assert(2 * FIELD_FC == 64, "fr_dgrad64_kernel");
        hipLaunchKernelGGL(fr_dgrad64_kernel, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, r->dp2, P + o.p2w, tw.p1, n, P2, r->dp1);
        wgrad(tw.d2, r->dp1, FIELD_FC, 2 * FIELD_FC, o.p1w);
        wgrad(tw.v1, r->dv2, 2 * FIELD_FC, FIELD_FC, o.v2w);
        dgrad(r->dv2, o.v2w, tw.v1, 2 * FIELD_FC, FIELD_FC, 0, r->dv1);
        wgrad(tw.d2, r->dv1, FIELD_FC, 2 * FIELD_FC, o.v1w);
        dgrad(r->dp1, o.p1w, nullptr, FIELD_FC, 2 * FIELD_FC, 0, r->dd2);
        dgrad(r->dv1, o.v1w, nullptr, FIELD_FC, 2 * FIELD_FC, 1, r->dd2);
        hipLaunchKernelGGL(field_relu_mask_kernel, dim3(nb(n * FIELD_FC)), dim3(256), 0, st, tw.d2, n * FIELD_FC, r->dd2);
        wgrad(tw.d1, r->dd2, 2 * FIELD_FC, FIELD_FC, o.d2w);
        dgrad(r->dd2, o.d2w, tw.d1, 2 * FIELD_FC, FIELD_FC, 0, r->dd1);
        wgrad(tw.x[net->L], r->dd1, net->D0, 2 * FIELD_FC, o.d1w);
        dgrad(r->dd1, o.d1w, nullptr, net->D0, 2 * FIELD_FC, 0, r->dxl[net->L]);
        for (int l = net->L - 1; l >= 0; --l) {
            const int H = net->lh[l], Wd = net->lw[l], Cin = net->lc[l], F = net->F;
            const long conv = n * H * Wd * F;
            const int Tw = 9 * Cin * F + F;
            hipLaunchKernelGGL(field_pool_bwd_kernel, dim3(nb(conv)), dim3(256), 0, st, r->dxl[l + 1], tw.x[l + 1], tw.idx[l], conv, H, Wd, F, r->dzc);
            hipLaunchKernelGGL(field_conv_wgrad_kernel, dim3((unsigned)n), dim3(256), 0, st, tw.x[l], r->dzc, H, Wd, Cin, F, r->cslab);
            hipLaunchKernelGGL(fr_rows_partial_kernel, dim3(nb(Tw), splits), dim3(256), 0, st, r->cslab, n, Tw, r->slab);
            hipLaunchKernelGGL(fr_accum_kernel, dim3(nb(Tw)), dim3(256), 0, st, r->slab, splits, Tw, Gr + o.cw[l]);
            if (l > 0) {
                const long tin = n * H * Wd * Cin;
                hipLaunchKernelGGL(field_conv_dgrad_kernel, dim3(nb(tin)), dim3(256), 0, st, r->dzc, P + o.cw[l], tin, H, Wd, Cin, F, r->dxl[l]);
            }
        }
    }
    const int nparts = 1024;
    hipLaunchKernelGGL(paac_sumsq_kernel<>, dim3(nparts), dim3(256), 0, st, Gr, o.total, net->stats64 + 8);
    hipLaunchKernelGGL(field_finalize_kernel, dim3(1), dim3(64), 0, st, net->stats64 + 8, nparts, net->stats64, inv_n, net->cfg.clip_norm, net->stats);
    if (finish) {
        net->adam_t += 1;
        net->param_version += 1;
        hipLaunchKernelGGL(paac_adam_kernel<>, dim3(nb(o.total)), dim3(256), 0, st, net->params, Gr, net->adam_m, net->adam_v, o.total, net->stats,
                           adam_lr_t(lr, net->adam_t));
    }
    PAAC_HIP(net, hipGetLastError());
    PAAC_HIP(net, hipStreamSynchronize(st));
    return paac_read_stats(net, stats_host);
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_fieldnet_rollout_bind(grl_fieldnet *net, float gamma) {
    if (!net || !(gamma >= 0.f) || !(gamma <= 1.f)) return paac_fail(net, GRL_E_INVALID, "grl_fieldnet_rollout_bind: bad argument");
    int rc = fr_check(net, "grl_fieldnet_rollout_bind");
    if (rc) return rc;
    if (!net->ro) net->ro = new FieldRollout();
    net->ro->gamma = gamma;
    return GRL_OK;
}

int grl_fieldnet_predict_swarm(grl_fieldnet *net, float *mu_host, float *sigma_host, float *vs_host) {
    if (!net) return GRL_E_INVALID;
    int rc = fr_prepare(net, "grl_fieldnet_predict_swarm");
    if (rc) return rc;
    FieldRollout *r = net->ro;
    FieldStepArgs a{};
    a.mu = r->cur_mu; a.sigma = r->cur_sg; a.vs = r->cur_vs;
    if ((rc = fr_forward_current(net, a))) return rc;
    PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
    const size_t B = (size_t)net->h->E * FR_AGENTS;
    if (mu_host) PAAC_HIP(net, hipMemcpy(mu_host, r->cur_mu, B * FR_A * 4, hipMemcpyDeviceToHost));
    if (sigma_host) PAAC_HIP(net, hipMemcpy(sigma_host, r->cur_sg, B * FR_A * 4, hipMemcpyDeviceToHost));
    if (vs_host) PAAC_HIP(net, hipMemcpy(vs_host, r->cur_vs, B * 4, hipMemcpyDeviceToHost));
    return GRL_OK;
}

int grl_fieldnet_debug_grid(grl_fieldnet *net, int32_t n_envs, const uint8_t *locust_bins, const uint8_t *agent_bins, float *states_host, size_t bytes) {
    if (!net || n_envs <= 0 || !locust_bins || !agent_bins || !states_host) return paac_fail(net, GRL_E_INVALID, "grl_fieldnet_debug_grid: bad argument");
    int rc = fr_check(net, "grl_fieldnet_debug_grid");
    if (rc) return rc;
    const int G = net->cfg.height;
    const size_t need = (size_t)n_envs * G * G * 2 * sizeof(float);
    if (bytes != need) return paac_fail(net, GRL_E_SIZE, "grl_fieldnet_debug_grid: states need " + std::to_string(need) + " bytes");
    hipSetDevice(net->h->cfg.device_id);
    hipStream_t st = net->h->stream;
    uint8_t *buf = nullptr;
    const size_t nl = (size_t)n_envs * 160, na = (size_t)n_envs * 20, off = (nl + na + 255) & ~(size_t)255;
    PAAC_HIP(net, hipMalloc((void **)&buf, off + need));
    hipError_t e = hipMemcpyAsync(buf, locust_bins, nl, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(buf + nl, agent_bins, na, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(field_grid_kernel, dim3(n_envs), dim3(256), 0, st, buf, buf + nl, G, reinterpret_cast<float *>(buf + off));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(states_host, buf + off, need, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return paac_fail(net, GRL_E_HIP, std::string("grl_fieldnet_debug_grid: ") + hipGetErrorString(e));
    return GRL_OK;
}

int grl_fieldnet_rollout(grl_fieldnet *net, int32_t T, int32_t reward_layout) {
    if (!net || T <= 0 || T > 1024 || (reward_layout != 0 && reward_layout != 1)) return paac_fail(net, GRL_E_INVALID, "grl_fieldnet_rollout: bad argument");
    int rc = fr_prepare(net, "grl_fieldnet_rollout");
    if (rc) return rc;
    if ((rc = fr_ensure_rollout_bufs(net, T))) return rc;
    FieldRollout *r = net->ro;
    grl_handle *h = net->h;
    hipStream_t st = h->stream;
    const int E = h->E;
    const size_t B = (size_t)E * FR_AGENTS;
    r->T = T;
    if (reward_layout == 1) PAAC_HIP(net, hipMemsetAsync(r->ro_rew, 0, (size_t)T * B * 4, st));
    const unsigned long counter0 = net->act_counter;
    net->act_counter += (unsigned long)T;
    for (int t = 0; t <= T; ++t) {
        FieldStepArgs a{};
        if (t == T) {      // bootstrap value of the state after the last step (paac.py:351-358)
            a.mu = r->cur_mu; a.sigma = r->cur_sg; a.vs = r->ro_boot;
            if ((rc = fr_forward_current(net, a))) return rc;
            break;
        }
        a.mu = r->ro_mu + (size_t)t * B * FR_A; a.sigma = r->ro_sg + (size_t)t * B * FR_A; a.vs = r->ro_val + (size_t)t * B;
        a.raw = r->ro_act + (size_t)t * B * FR_A; a.envact = r->ro_envact + (size_t)t * B * FR_A;
        a.counter = (uint32_t)(counter0 + (unsigned long)t);
        // states[t] = shared_states (paac.py:319): the compact observation the action was chosen from
        a.ro_lb = reinterpret_cast<uint32_t *>(r->ro_lb + (size_t)t * E * 160);
        a.ro_ab = reinterpret_cast<uint32_t *>(r->ro_ab + (size_t)t * E * 20);
        a.ro_pos = reinterpret_cast<uint32_t *>(r->ro_pos + (size_t)t * E * 20);
        if ((rc = fr_forward_current(net, a))) return rc;
        if ((rc = swarm_launch_step_range(h, a.envact, 0, E, 0, true)) || (rc = episodes_launch_account(h, 0, E)))      // R6 (paac.py:331-349)
            return paac_fail(net, rc, h->err);
        hipLaunchKernelGGL(field_reward_layout_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, h->reward, E, reward_layout,
                           r->ro_rew + (size_t)t * B, (const uint8_t *)h->done, r->ro_done + (size_t)t * E);
    }
    // n-step returns over all columns (paac.py:360-372)
    if ((rc = launch_returns(h, r->ro_rew, r->ro_val, nullptr, r->ro_boot, T, (int)B, r->gamma, 1.0f, net->cfg.scale, 0.f, 0.f, r->ro_y, r->ro_adv)))
        return paac_fail(net, rc, h->err);
    PAAC_HIP(net, hipGetLastError());
    h->step_in_flight = true;
    return GRL_OK;
}

int grl_fieldnet_train_rollout(grl_fieldnet *net, float lr, float *stats_host) { return fr_train(net, lr, stats_host, 1); }
int grl_fieldnet_train_rollout_grads(grl_fieldnet *net, float *stats_host) { return fr_train(net, 0.f, stats_host, 0); }

int grl_fieldnet_read_rollout(grl_fieldnet *net, const char *which, void *host, size_t bytes) {
    if (!net || !which || !host) return GRL_E_INVALID;
    if (!net->ro || net->ro->T <= 0) return paac_fail(net, GRL_E_STATE, "grl_fieldnet_read_rollout: no rollout yet");
    hipSetDevice(net->h->cfg.device_id);
    const FieldRollout *r = net->ro;
    const std::string w(which);
    const size_t T = r->T, E = net->h->E, B = E * FR_AGENTS;
    const struct { const char *name; const void *src; size_t need; } table[] = {
        {"actions", r->ro_act, T * B * 8}, {"env_actions", r->ro_envact, T * B * 8}, {"mu", r->ro_mu, T * B * 8}, {"sigma", r->ro_sg, T * B * 8},
        {"values", r->ro_val, T * B * 4}, {"rewards", r->ro_rew, T * B * 4}, {"y", r->ro_y, T * B * 4}, {"adv", r->ro_adv, T * B * 4},
        {"boot", r->ro_boot, B * 4}, {"dones", r->ro_done, T * E}, {"locust_bins", r->ro_lb, T * E * 160}, {"agent_bins", r->ro_ab, T * E * 20},
        {"positions", r->ro_pos, T * E * 20}};
    for (const auto &e : table) {
        if (w != e.name) continue;
        if (e.need != bytes) return paac_fail(net, GRL_E_SIZE, "grl_fieldnet_read_rollout: '" + w + "' needs " + std::to_string(e.need) + " bytes");
        PAAC_HIP(net, hipStreamSynchronize(net->h->stream));
        PAAC_HIP(net, hipMemcpy(host, e.src, bytes, hipMemcpyDeviceToHost));
        return GRL_OK;
    }
    return paac_fail(net, GRL_E_INVALID, "grl_fieldnet_read_rollout: unknown buffer '" + w + "'");
}

int grl_fieldnet_get_optimizer_state(grl_fieldnet *net, float *m_host, float *v_host, int64_t n, int64_t *step_out) {
    return paac_get_optimizer_state(net, m_host, v_host, n, step_out);
}
int grl_fieldnet_set_optimizer_state(grl_fieldnet *net, const float *m_host, const float *v_host, int64_t n, int64_t step) {
    return paac_set_optimizer_state(net, "grl_fieldnet_set_optimizer_state", m_host, v_host, n, step);
}
int grl_fieldnet_get_action_counter(grl_fieldnet *net, uint64_t *out) { return paac_get_action_counter(net, out); }
int grl_fieldnet_set_action_counter(grl_fieldnet *net, uint64_t value) { return paac_set_action_counter(net, value); }

}  // extern "C"
