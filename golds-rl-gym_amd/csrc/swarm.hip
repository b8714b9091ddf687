// Swarm-v0 on gfx950: SwarmEnv._step / _reset (reference fed_gym/envs/multiagent.py:30-115),
// gym TimeLimit, and SwarmStateProcessor.process_state (fed_gym/agents/state_processors.py:17-42)
// as hand-written HIP.
//
// Mapping: one lane per locust, 4 envs per 320-lane workgroup (5 full waves, no idle lanes);
// the 90 source points of each env (80 locusts + 10 agents, float64 x/y interleaved) live in LDS
// and are read as wave-broadcast ds_read_b128; each lane runs the 90-term force sum for its own
// locust in the reference's (numpy pairwise) association order, so no cross-lane reduction is
// needed for v.  Agents are advanced by the first 40 lanes.  The observation (bin indices) is
// produced by the same launch from the positions already in LDS/registers; the dense 84x84 image
// is never written.  HBM traffic per env-step: x 1280 + xa 160 + noise rows 1440 +
// actions 80 read; x 1280 + xa 160 + bins 200 + reward/done/elapsed ~17 written.
#include "common.h"
#include "rng.h"
#include "swarm_dev.h"
#include <stdlib.h>
#include <string.h>

namespace grl {

struct SwarmParams {
    double *x, *xa, *pnoise, *anoise;
    const double *rx, *rxa, *rpn, *ran;               // reset snapshot
    const double *inj_x0, *inj_xa0, *inj_ra, *inj_an, *inj_pn;  // injected reset draws
    const float *actions;
    const double *actions64;     // if set: float64 actions (SwarmEnv.step called directly, e.g. by the eval monitor) instead of `actions`
    int32_t *elapsed, *episode;
    float *reward;
    double *reward64;
    uint8_t *done, *lbins, *abins, *pos;
    int32_t *done_list, *done_count;
    const int32_t *reset_list, *reset_count;
    int E, grid, max_steps;
    int env_base;                // MODE_STEP / MODE_OBSERVE: the launch covers envs [env_base, E) (E = end of the range)
    uint32_t flags, env_off;
    uint64_t seed;
    int no_wind;                 // MODE_STEP: SwarmEnv._step(v_action, add_wind=False) -- the agents' action row is used as it is (multiagent.py:33-36)
};

enum { MODE_STEP = 0, MODE_OBSERVE = 1, MODE_RESET = 2 };

// The body of swarm_kernel / swarm_kernel_refdiv; MATH selects pair_term's arithmetic.
template <int MODE, int MATH>
__device__ __forceinline__ void swarm_body(const SwarmParams &P) {
    __shared__ SwarmLds L;
    __shared__ int env_of[SWARM_EPB];
    const int tid = threadIdx.x;
    const int el = tid / N_LOCUSTS, j = tid - el * N_LOCUSTS;

    if (MODE == MODE_RESET) {
        int cnt = *P.reset_count;
        if ((int)blockIdx.x * SWARM_EPB >= cnt) return;   // block-uniform
        if (tid < SWARM_EPB) {
            int li = blockIdx.x * SWARM_EPB + tid;
            env_of[tid] = li < cnt ? P.reset_list[li] : -1;
        }
    } else {
        if (tid < SWARM_EPB) {
            int e = P.env_base + blockIdx.x * SWARM_EPB + tid;
            env_of[tid] = e < P.E ? e : -1;
        }
    }
    __syncthreads();
    const int env = env_of[el];
    const bool active = env >= 0;
    const int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;   // agent-lane view (valid when tid < 40)
    const bool agent_lane = tid < SWARM_EPB * N_AGENTS;
    const int aenv = agent_lane ? env_of[ea] : -1;
    const bool aactive = aenv >= 0;

    double xj = 0.5, yj = 0.5;
    if (MODE == MODE_STEP || MODE == MODE_OBSERVE) {
        if (active) {
            double2 q = reinterpret_cast<const double2 *>(P.x)[(size_t)env * N_LOCUSTS + j];
            xj = q.x; yj = q.y;
        }
        if (agent_lane) {
            double2 q = make_double2(0.5, 0.5);
            if (aactive) q = reinterpret_cast<const double2 *>(P.xa)[(size_t)aenv * N_AGENTS + a];
            L.p[ea][N_LOCUSTS + a] = q;
        }
    }

    if (MODE == MODE_STEP) {
        double actx = 0, acty = 0, anx = 0, any = 0, pnx = 0, pny = 0;
        if (active) {
            double2 n = reinterpret_cast<const double2 *>(P.pnoise)[(size_t)env * N_LOCUSTS + j];
            pnx = n.x; pny = n.y;
        }
        if (aactive) {
            if (P.actions64) {
                double2 act = reinterpret_cast<const double2 *>(P.actions64)[(size_t)aenv * N_AGENTS + a];
                actx = act.x; acty = act.y;
            } else {
                float2 act = reinterpret_cast<const float2 *>(P.actions)[(size_t)aenv * N_AGENTS + a];
                actx = (double)act.x; acty = (double)act.y;
            }
            double2 n = reinterpret_cast<const double2 *>(P.anoise)[(size_t)aenv * N_AGENTS + a];
            anx = n.x; any = n.y;
        }
        block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny, P.actions64 == nullptr, P.no_wind == 0);
        if (active) reinterpret_cast<double2 *>(P.x)[(size_t)env * N_LOCUSTS + j] = make_double2(xj, yj);
        if (aactive) reinterpret_cast<double2 *>(P.xa)[(size_t)aenv * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
        if (active && j == 0) {
            double r = L.rew[el];
            int el_new = P.elapsed[env] + 1;            // gym TimeLimit: counts wrapped steps
            bool d = (r >= 0) || (P.max_steps > 0 && el_new >= P.max_steps);   // multiagent.py:44 + TimeLimit
            P.elapsed[env] = el_new;
            P.reward64[env] = r;
            P.reward[env] = (float)r;
            P.done[env] = d ? 1 : 0;
            L.dflag[el] = d ? env : -1;
        } else if (j == 0) {
            L.dflag[el] = -1;
        }
        // episode-done compaction (emulator_runner.py:128-132 resets exactly these): the workgroup's finished envs take ONE slot
        // range with one atomicAdd (at a TimeLimit boundary every env of the batch finishes in the same launch); the order of
        // the list across workgroups is arrival order, grl_read_output("done_list") sorts it
        __syncthreads();
        if (tid == 0) {
            int n = 0;
#pragma unroll
            for (int e = 0; e < SWARM_EPB; ++e) n += L.dflag[e] >= 0 ? 1 : 0;
            if (n) {
                int slot = atomicAdd(P.done_count, n);
#pragma unroll
                for (int e = 0; e < SWARM_EPB; ++e)
                    if (L.dflag[e] >= 0) P.done_list[slot++] = L.dflag[e];
            }
        }
    }

    if (MODE == MODE_RESET) {
        const uint32_t genv = active ? (uint32_t)env + P.env_off : 0u;
        const uint32_t gaenv = aactive ? (uint32_t)aenv + P.env_off : 0u;
        const uint32_t ep = (active && !(P.flags & GRL_F_RESEED_EACH_RESET)) ? (uint32_t)P.episode[env] : 0u;
        const uint32_t aep = (aactive && !(P.flags & GRL_F_RESEED_EACH_RESET)) ? (uint32_t)P.episode[aenv] : 0u;
        double pn10x = 0, pn10y = 0, an10x = 0, an10y = 0;
        if (P.flags & GRL_F_RESET_FROM_SNAPSHOT) {
            if (active) {
                double2 q = reinterpret_cast<const double2 *>(P.rx)[(size_t)env * N_LOCUSTS + j];
                xj = q.x; yj = q.y;
                double2 n = reinterpret_cast<const double2 *>(P.rpn)[(size_t)env * N_LOCUSTS + j];
                pn10x = n.x; pn10y = n.y;
            }
            if (agent_lane) {
                double2 q = make_double2(0.5, 0.5);
                if (aactive) {
                    q = reinterpret_cast<const double2 *>(P.rxa)[(size_t)aenv * N_AGENTS + a];
                    double2 n = reinterpret_cast<const double2 *>(P.ran)[(size_t)aenv * N_AGENTS + a];
                    an10x = n.x; an10y = n.y;
                }
                L.p[ea][N_LOCUSTS + a] = q;
            }
            L.p[el][j] = make_double2(xj, yj);
            __syncthreads();
        } else {
            const bool inj = P.inj_x0 != nullptr;
            // x ~ U[0,1)^(80,2), xa ~ U[0,1)^(10,2)  (multiagent.py:51-52)
            if (inj) {
                if (active) {
                    double2 q = reinterpret_cast<const double2 *>(P.inj_x0)[(size_t)env * N_LOCUSTS + j];
                    xj = q.x; yj = q.y;
                }
            } else {
                u01_pair(rng_block(P.seed, genv, ep, RS_SWARM_X0, j), xj, yj);
            }
            if (agent_lane) {
                double2 q = make_double2(0.5, 0.5);
                if (inj) {
                    if (aactive) q = reinterpret_cast<const double2 *>(P.inj_xa0)[(size_t)aenv * N_AGENTS + a];
                } else {
                    u01_pair(rng_block(P.seed, gaenv, aep, RS_SWARM_XA0, a), q.x, q.y);
                }
                L.p[ea][N_LOCUSTS + a] = q;
            }
            // N_BURN_IN steps with noise rows 0..9 (multiagent.py:58-61), then row 10 is kept (quirk Q1)
            for (int t = 0; t <= N_BURN_IN; ++t) {
                double actx = 0, acty = 0, anx = 0, any = 0, pnx = 0, pny = 0;
                if (inj) {
                    if (active) {
                        double2 n = reinterpret_cast<const double2 *>(P.inj_pn)[((size_t)env * (N_BURN_IN + 1) + t) * N_LOCUSTS + j];
                        pnx = n.x; pny = n.y;
                    }
                    if (aactive) {
                        double2 n = reinterpret_cast<const double2 *>(P.inj_an)[((size_t)aenv * (N_BURN_IN + 1) + t) * N_AGENTS + a];
                        anx = n.x; any = n.y;
                        if (t < N_BURN_IN) {
                            double2 r = reinterpret_cast<const double2 *>(P.inj_ra)[((size_t)aenv * N_BURN_IN + t) * N_AGENTS + a];
                            actx = r.x; acty = r.y;
                        }
                    }
                } else {
                    normal_pair(rng_block(P.seed, genv, ep, RS_SWARM_PNOISE, t * N_LOCUSTS + j), pnx, pny);
                    if (agent_lane) {
                        normal_pair(rng_block(P.seed, gaenv, aep, RS_SWARM_ANOISE, t * N_AGENTS + a), anx, any);
                        if (t < N_BURN_IN) normal_pair(rng_block(P.seed, gaenv, aep, RS_SWARM_RANDACT, t * N_AGENTS + a), actx, acty);
                    }
                }
                if (t == N_BURN_IN) {
                    pn10x = pnx; pn10y = pny; an10x = anx; an10y = any;
                    break;
                }
                block_step<MATH>(L, tid, el, j, xj, yj, actx, acty, anx, any, pnx, pny);
            }
        }
        if (active) {
            reinterpret_cast<double2 *>(P.x)[(size_t)env * N_LOCUSTS + j] = make_double2(xj, yj);
            reinterpret_cast<double2 *>(P.pnoise)[(size_t)env * N_LOCUSTS + j] = make_double2(pn10x, pn10y);
            if (j == 0) {
                P.elapsed[env] = 0;
                P.episode[env] = P.episode[env] + 1;
            }
        }
        if (aactive) {
            reinterpret_cast<double2 *>(P.xa)[(size_t)aenv * N_AGENTS + a] = L.p[ea][N_LOCUSTS + a];
            reinterpret_cast<double2 *>(P.anoise)[(size_t)aenv * N_AGENTS + a] = make_double2(an10x, an10y);
        }
    }

    if (MODE == MODE_OBSERVE) {
        L.p[el][j] = make_double2(xj, yj);
        __syncthreads();
    }

    // ---- observation: process_state (state_processors.py:29-42) -------------------------------
    if (P.flags & GRL_F_SWARM_NO_OBSERVE) return;
    if (j == 0) L.meanx[el] = swarm_mean_x(L.p[el]);
    __syncthreads();
    const int G = P.grid;
    {
        int cx, cy;
        const uint16_t bin = swarm_point_bin(xj, yj, L.meanx[el], G, cx, cy);
        if (active) reinterpret_cast<uint16_t *>(P.lbins)[(size_t)env * N_LOCUSTS + j] = bin;
    }
    if (aactive) {
        const double2 q = L.p[ea][N_LOCUSTS + a];
        int cx, cy;
        reinterpret_cast<uint16_t *>(P.abins)[(size_t)aenv * N_AGENTS + a] = swarm_point_bin(q.x, q.y, L.meanx[ea], G, cx, cy);
        reinterpret_cast<uint16_t *>(P.pos)[(size_t)aenv * N_AGENTS + a] = swarm_point_pos(cx, cy, G);
    }
}

template <int MODE, bool FAST>
// The step's pair loop is a long chain of dependent fp64 operations (two exp polynomials, three quotients per pair): five waves per SIMD
// instead of the four its 124 registers allowed hide more of it -- 0.976 -> 0.875 ms per 32 768-env step with 96 registers and 24 bytes of
// scratch per lane (round 4).  Six waves (80 registers, 104 bytes of scratch) measured 0.859 ms but tripled the kernel's HBM-side bytes
// (each lane writes and reads its spill slots once: 488 MB per launch against 151 MB algorithmic); 7 / 8 waves: 0.875 / 0.863 ms.
// With the quotients from one reciprocal (pair_term<MATH_EXACT>): 276 -> 217 us per 8 192-env chunk, 96 registers, 20 bytes of scratch.
// The second launch bound is waves per SIMD.
__global__ __launch_bounds__(SWARM_TPB, MODE == 0 ? 5 : 1) void swarm_kernel(SwarmParams P) {
    swarm_body<MODE, FAST ? MATH_FAST : MATH_EXACT>(P);
}

// GRL_SWARM_DIV=ref: the exact path with the compiler's three IEEE divisions per pair, for tests/test_gpu_swarm_div.py
template <int MODE>
__global__ __launch_bounds__(SWARM_TPB, MODE == 0 ? 5 : 1) void swarm_kernel_refdiv(SwarmParams P) {
    swarm_body<MODE, MATH_REFDIV>(P);
}

// get_local_states (paac/emulator_runner.py:98-111) as a dense f32 tensor; compat/debug only.
__global__ void swarm_materialize_kernel(const uint8_t *lbins, const uint8_t *abins, const uint8_t *pos, int first, int G,
                                         float *out) {
    extern __shared__ unsigned int cnt[];   // [2][G*G]
    const int env = first + blockIdx.x;
    const int GG = G * G;
    for (int i = threadIdx.x; i < 2 * GG; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    if (threadIdx.x < N_LOCUSTS) {
        int bx = lbins[((size_t)env * N_LOCUSTS + threadIdx.x) * 2], by = lbins[((size_t)env * N_LOCUSTS + threadIdx.x) * 2 + 1];
        if (bx != 255) atomicAdd(&cnt[bx * G + by], 1u);
    } else if (threadIdx.x < N_POINTS) {
        int a = threadIdx.x - N_LOCUSTS;
        int bx = abins[((size_t)env * N_AGENTS + a) * 2], by = abins[((size_t)env * N_AGENTS + a) * 2 + 1];
        if (bx != 255) atomicAdd(&cnt[GG + bx * G + by], 1u);
    }
    __syncthreads();
    float *o = out + (size_t)blockIdx.x * N_AGENTS * GG * 3;
    for (int a = 0; a < N_AGENTS; ++a) {
        int px = pos[((size_t)env * N_AGENTS + a) * 2], py = pos[((size_t)env * N_AGENTS + a) * 2 + 1];
        int hot = px * G + py;
        for (int i = threadIdx.x; i < GG * 3; i += blockDim.x) {
            int pix = i / 3, c = i - pix * 3;
            float v;
            if (c == 0) v = (float)((double)cnt[pix] / 80.0);          // x_grid / len(state[0])
            else if (c == 1) v = (float)((double)cnt[GG + pix] / 10.0);  // xa_grid / len(state[1])
            else v = (pix == hot) ? 1.0f : 0.0f;
            o[(size_t)a * GG * 3 + i] = v;
        }
    }
}

static SwarmParams make_params(grl_handle *h) {
    SwarmParams P{};
    P.x = h->sw.x; P.xa = h->sw.xa; P.pnoise = h->sw.pnoise; P.anoise = h->sw.anoise;
    P.rx = h->sw.rx; P.rxa = h->sw.rxa; P.rpn = h->sw.rpnoise; P.ran = h->sw.ranoise;
    P.elapsed = h->elapsed; P.episode = h->episode; P.reward = h->reward; P.reward64 = h->sw.reward64;
    P.done = h->done; P.lbins = h->sw.lbins; P.abins = h->sw.abins; P.pos = h->sw.pos;
    P.done_list = h->done_list; P.done_count = h->done_count;
    P.E = h->E; P.grid = h->cfg.grid_size; P.max_steps = h->cfg.max_episode_steps;
    P.flags = h->cfg.flags; P.env_off = (uint32_t)h->cfg.env_id_offset; P.seed = h->cfg.seed;
    return P;
}

template <typename T>
static int dmalloc(grl_handle *h, T **p, size_t n) {
    GRL_HIP(h, hipMalloc((void **)p, n * sizeof(T)));
    h->allocs.push_back(*p);
    GRL_HIP(h, hipMemsetAsync(*p, 0, n * sizeof(T), h->stream));
    return GRL_OK;
}

int swarm_alloc(grl_handle *h) {
    size_t E = h->E;
    int rc;
    { const char *dv = getenv("GRL_SWARM_DIV"); h->sw.ref_div = dv && strcmp(dv, "ref") == 0; }      // A/B and tests: pair_term's MATH_REFDIV
    if ((rc = dmalloc(h, &h->sw.x, E * N_LOCUSTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.xa, E * N_AGENTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.pnoise, E * N_LOCUSTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.anoise, E * N_AGENTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.reward64, E))) return rc;
    if ((rc = dmalloc(h, &h->sw.lbins, E * N_LOCUSTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.abins, E * N_AGENTS * 2))) return rc;
    if ((rc = dmalloc(h, &h->sw.pos, E * N_AGENTS * 2))) return rc;
    if (h->cfg.flags & GRL_F_RESET_FROM_SNAPSHOT) {
        if ((rc = dmalloc(h, &h->sw.rx, E * N_LOCUSTS * 2))) return rc;
        if ((rc = dmalloc(h, &h->sw.rxa, E * N_AGENTS * 2))) return rc;
        if ((rc = dmalloc(h, &h->sw.rpnoise, E * N_LOCUSTS * 2))) return rc;
        if ((rc = dmalloc(h, &h->sw.ranoise, E * N_AGENTS * 2))) return rc;
    }
    return GRL_OK;
}

static inline int nblocks(int n) { return (n + SWARM_EPB - 1) / SWARM_EPB; }

// the step / reset kernel in the handle's arithmetic: fast math, the exact path, or the exact path with the reference divisions
template <int MODE>
static void launch_swarm(grl_handle *h, int blocks, const SwarmParams &P) {
    if (h->cfg.flags & GRL_F_SWARM_FAST_MATH)
        hipLaunchKernelGGL((swarm_kernel<MODE, true>), dim3(blocks), dim3(SWARM_TPB), 0, h->stream, P);
    else if (h->sw.ref_div)
        hipLaunchKernelGGL((swarm_kernel_refdiv<MODE>), dim3(blocks), dim3(SWARM_TPB), 0, h->stream, P);
    else
        hipLaunchKernelGGL((swarm_kernel<MODE, false>), dim3(blocks), dim3(SWARM_TPB), 0, h->stream, P);
}

int swarm_launch_step(grl_handle *h, const float *actions_dev, const double *actions64_dev, int no_wind) {
    SwarmParams P = make_params(h);
    P.actions = actions_dev;
    P.actions64 = actions64_dev;
    P.no_wind = no_wind;
    GRL_HIP(h, hipMemsetAsync(h->done_count, 0, sizeof(int32_t), h->stream));
    prof_begin(h);
    launch_swarm<MODE_STEP>(h, nblocks(h->E), P);
    prof_end(h);
    GRL_HIP(h, hipGetLastError());
    // auto-reset of the envs that just finished (paac/emulator_runner.py:128-132): the terminal
    // reward/done stay, the observation becomes the reset one (quirk Q6)
    return swarm_launch_reset(h, h->done_list, h->done_count, h->E);
}

// The step for envs [env_base, env_base + count) only, enqueued on the handle's CURRENT stream: the rollout of the conv policy
// runs every chunk of envs as its own pipeline (forward -> sample -> step -> bookkeeping) on one of a few streams, so the fp64
// VALU-bound step of one chunk overlaps the MFMA GEMMs of the others.  `slot` < 16 selects the done counter (one per stream; the
// finished envs of the range are listed at done_list + env_base).
int swarm_launch_step_range(grl_handle *h, const float *actions_dev, int env_base, int count, int slot, bool counter_zeroed) {
    SwarmParams P = make_params(h);
    P.actions = actions_dev;
    P.actions64 = nullptr;
    P.env_base = env_base;
    P.E = env_base + count;
    P.done_list = h->done_list + env_base;
    P.done_count = h->done_count + slot;
    if (!counter_zeroed) GRL_HIP(h, hipMemsetAsync(P.done_count, 0, sizeof(int32_t), h->stream));      // (the conv rollout's sampling kernel does it)
    launch_swarm<MODE_STEP>(h, nblocks(count), P);
    GRL_HIP(h, hipGetLastError());
    return swarm_launch_reset(h, P.done_list, P.done_count, count);
}

int swarm_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count) {
    SwarmParams P = make_params(h);
    P.reset_list = list_dev;
    P.reset_count = count_dev;
    launch_swarm<MODE_RESET>(h, nblocks(max_count), P);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

int swarm_launch_observe(grl_handle *h) {
    SwarmParams P = make_params(h);
    P.flags &= ~GRL_F_SWARM_NO_OBSERVE;
    hipLaunchKernelGGL((swarm_kernel<MODE_OBSERVE, false>), dim3(nblocks(h->E)), dim3(SWARM_TPB), 0, h->stream, P);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

int swarm_reset_injected(grl_handle *h, const double *x0, const double *xa0, const double *ra, const double *an,
                         const double *pn) {
    size_t E = h->E;
    size_t n_x0 = E * N_LOCUSTS * 2, n_xa0 = E * N_AGENTS * 2, n_ra = E * N_BURN_IN * N_AGENTS * 2;
    size_t n_an = E * (N_BURN_IN + 1) * N_AGENTS * 2, n_pn = E * (N_BURN_IN + 1) * N_LOCUSTS * 2;
    double *buf = nullptr;
    GRL_HIP(h, hipMalloc((void **)&buf, (n_x0 + n_xa0 + n_ra + n_an + n_pn) * sizeof(double)));
    double *d_x0 = buf, *d_xa0 = d_x0 + n_x0, *d_ra = d_xa0 + n_xa0, *d_an = d_ra + n_ra, *d_pn = d_an + n_an;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(d_x0, x0, n_x0 * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_xa0, xa0, n_xa0 * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ra, ra, n_ra * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_an, an, n_an * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pn, pn, n_pn * 8, hipMemcpyHostToDevice, h->stream);
    int rc = GRL_OK;
    if (e == hipSuccess) {
        rc = launch_iota(h, h->done_list, h->E);
        int32_t cnt = h->E;
        if (rc == GRL_OK) e = hipMemcpyAsync(h->done_count, &cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream);
        if (rc == GRL_OK && e == hipSuccess) {
            e = hipStreamSynchronize(h->stream);   // cnt is a stack variable
            SwarmParams P = make_params(h);
            P.flags &= ~(GRL_F_RESET_FROM_SNAPSHOT);
            P.reset_list = h->done_list; P.reset_count = h->done_count;
            P.inj_x0 = d_x0; P.inj_xa0 = d_xa0; P.inj_ra = d_ra; P.inj_an = d_an; P.inj_pn = d_pn;
            launch_swarm<MODE_RESET>(h, nblocks(h->E), P);
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
    }
    hipFree(buf);
    if (rc != GRL_OK) return rc;
    if (e != hipSuccess) return hip_fail(h, e, "swarm_reset_injected");
    return GRL_OK;
}

int swarm_materialize(grl_handle *h, int first, int count, float *out_dev) {
    int G = h->cfg.grid_size;
    size_t lds = (size_t)2 * G * G * sizeof(unsigned int);
    hipLaunchKernelGGL(swarm_materialize_kernel, dim3(count), dim3(256), lds, h->stream, h->sw.lbins, h->sw.abins,
                       h->sw.pos, first, G, out_dev);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

}  // namespace grl
