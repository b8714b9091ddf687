// Device-side Swarm arithmetic shared by the translation units that step a Swarm env (swarm.hip: the step / reset / observe kernels,
// swarm_replay.hip / swarm_rules.hip: whole scripted or rule-driven episodes in one launch, net_field_eval.inc: the field policy's): the
// workgroup's LDS layout, the constants of envs/multiagent.py, SwarmEnv._step for the 4 envs of a 320-lane workgroup (block_step) and the
// compact observation of one point.  Every file is compiled with -ffp-contract=off.
#pragma once
#include <type_traits>

#include "common.h"

namespace grl {

constexpr int LDS_STRIDE = 97;   // 90 points padded so two envs' rows start on different banks

struct SwarmLds {
    double2 p[SWARM_EPB][LDS_STRIDE];
    double en[SWARM_EPB][N_LOCUSTS];
    double meanx[SWARM_EPB];
    double rew[SWARM_EPB];
    int dflag[SWARM_EPB];      // env id of a finished episode (or -1): folded into ONE atomicAdd per workgroup
};

constexpr double DT = 0.05, NOISE = 0.0001, WIND = 1.0, GRAV = -1.0, FATT = 0.5, LATT = 10.0;

// xv_cutoff (multiagent.py:77-86)
__device__ __forceinline__ void cutoff(double &y, double &vx, double &vy) {
    if (y <= 0) {
        y = 0;
        vx = 0;
        if (vy <= 0) vy = 0;
    }
}

// x_update (multiagent.py:70-75); n* are raw N(0,1) draws
__device__ __forceinline__ void x_update(double &x, double &y, double vx, double vy, double nx, double ny) {
    cutoff(y, vx, vy);
    x = x + (DT * vx + NOISE * nx);
    y = y + (DT * vy + NOISE * ny);
    if (y <= 0) y = 0;
}

// x_update for the agents when the action row is FLOAT32 -- what the worker reads from the learner's shared c_float array
// (quirk Q7; emulator_runner.py:126, paac.py:269).  numpy keeps the row's dtype through `v_action[:, 0] += WIND_SPEED`
// (multiagent.py:33-36) and through `dt * v` (a Python float times a float32 array is a float32 product with dt rounded to
// float32, multiagent.py:72); only the sum with the float64 noise is float64.  Pinned by tests/golden/swarm_runner.npz
// (SwarmRunner._run itself): evaluating the action term in float64 differs by ~6e-9 per step, which the chaotic dynamics amplify.
__device__ __forceinline__ void x_update_f32v(double &x, double &y, float vx, float vy, double nx, double ny) {
    if (y <= 0) {
        y = 0;
        vx = 0;
        if (vy <= 0) vy = 0;
    }
    x = x + ((double)(0.05f * vx) + NOISE * nx);
    y = y + ((double)(0.05f * vy) + NOISE * ny);
    if (y <= 0) y = 0;
}

// How pair_term evaluates the exact path's three quotients.  MATH_EXACT and MATH_REFDIV give the same bits (see pair_term);
// MATH_REFDIV keeps the compiler's three IEEE divisions so that tests can hold the two against each other (GRL_SWARM_DIV=ref).
enum { MATH_EXACT = 0, MATH_FAST = 1, MATH_REFDIV = 2 };

template <int MATH>
__device__ __forceinline__ void pair_term(double sx, double sy, double xj, double yj, double &t0, double &t1) {
    double dx = sx - xj, dy = sy - yj;
    double d = sqrt(dx * dx + dy * dy);
    if (MATH == MATH_FAST) {
        double t = exp(d * -0.1);
        double t2 = t * t, t4 = t2 * t2, t5 = t4 * t, t10 = t5 * t5;
        double w = (FATT * t - t10) / (d + 0.000001);
        t0 = w * dx;
        t1 = w * dy;
    } else if (MATH == MATH_REFDIV) {
        // s(r) = F*exp(-r/L) - exp(-r)   (multiagent.py:65-68); term = s*dx/(r+1e-6) (:103-104)
        double s = FATT * exp(-d / LATT) - exp(-d);
        double den = d + 0.000001;
        t0 = s * dx / den;
        t1 = s * dy / den;
    } else {
        // The same three correctly rounded quotients as MATH_REFDIV, from one reciprocal instead of three divisions.  An IEEE
        // fp64 division expands to div_scale x2, rcp, two Newton steps on the reciprocal, quotient, one residual correction
        // (div_fmas) and div_fixup.  Below is that sequence without the scaling and the fix-up, and with the reciprocal of den
        // shared by both numerators.  Scaling and fix-up only act when an operand or the quotient is zero, subnormal, infinite,
        // NaN or within ~2^100 of the exponent limits; here they are identities:
        //   den = d + 1e-6 lies in [1e-6, d_max + 1e-6]; |s| <= 1 and |dx|, |dy| <= d bound a numerator s*dx by d_max.
        //   A nonzero numerator is a normal number far from the limits as long as d stays below a few hundred: s = F exp(-d/10) -
        //   exp(-d) is ~0.5 exp(-d/10) there (2e-44 at d = 1e3; near its root at d ~ 0.77 it is a difference of two doubles of
        //   (0, 1), at least ~1e-17 unless exactly zero), and a nonzero dx is at least an ulp of a coordinate (~1e-19).  The claim
        //   is made for d <= ~5e3, where |s| >= 1e-218: beyond d ~ 7e3 s itself goes subnormal and the unscaled sequence may differ
        //   from `/` in the last bit.  Nothing bounds a locust's x in x_update, but an episode is at most max_episode_steps long
        //   (gym's TimeLimit; 128 for Swarm-v0), the reset puts all points into the unit box and a step moves a point by
        //   dt |v| with |v| <= 1 + 90: two points are never 5e3 apart.  (max_episode_steps = 0 lifts the cap: the long-range force is
        //   attractive, so the swarm stays together in practice, but past d ~ 7e3 a quotient may then differ from `/` in its last bit.)
        //   A zero numerator (dx = 0 or s = 0) gives a zero quotient, but +0 where the division gives -0 (fma(-den, -0, -0) =
        //   +0).  That sign reaches no result: a zero term only decides the sign of a sum whose other terms are all zero, and
        //   locust_velocity adds that sum to WIND or GRAV; -d / 10 only feeds exp().
        // -d / 10: q = n * rn(1/10), one residual correction with the exact divisor (Markstein); rn(0.1) is the correctly
        // rounded reciprocal of 10, for which the corrected quotient is correctly rounded for every n away from the limits.
        // Held to `/` on 10^7 random operands plus the edge values by tests/test_swarm_div_exact.py, and on the device by
        // tests/test_gpu_swarm_div.py.  The fmas are explicit: the file is compiled with -ffp-contract=off.
        double n10 = -d;
        double q10 = n10 * 0.1;
        q10 = __builtin_fma(__builtin_fma(-LATT, q10, n10), 0.1, q10);
        double s = FATT * exp(q10) - exp(-d);
        double den = d + 0.000001;
        double y = __builtin_amdgcn_rcp(den);
        y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
        y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
        double n0 = s * dx, n1 = s * dy;
        double q0 = n0 * y, q1 = n1 * y;
        t0 = __builtin_fma(__builtin_fma(-den, q0, n0), y, q0);
        t1 = __builtin_fma(__builtin_fma(-den, q1, n1), y, q1);
    }
}

// v_calculate for one target locust (multiagent.py:100-113).  Sums follow numpy's pairwise
// order for n=80 and n=10: 8 strided accumulators, a fixed tree, then the tail.
template <int MATH>
__device__ __forceinline__ void locust_velocity(const double2 *src, double xj, double yj, double &vx, double &vy) {
    double a0[8], a1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pair_term<MATH>(src[k].x, src[k].y, xj, yj, a0[k], a1[k]);
    for (int i = 8; i < N_LOCUSTS; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double t0, t1;
            pair_term<MATH>(src[i + k].x, src[i + k].y, xj, yj, t0, t1);
            a0[k] += t0;
            a1[k] += t1;
        }
    }
    double ll0 = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
    double ll1 = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
#pragma unroll
    for (int k = 0; k < 8; ++k) pair_term<MATH>(src[N_LOCUSTS + k].x, src[N_LOCUSTS + k].y, xj, yj, a0[k], a1[k]);
    double al0 = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
    double al1 = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
#pragma unroll
    for (int k = 8; k < N_AGENTS; ++k) {
        double t0, t1;
        pair_term<MATH>(src[N_LOCUSTS + k].x, src[N_LOCUSTS + k].y, xj, yj, t0, t1);
        al0 += t0;
        al1 += t1;
    }
    vx = (WIND + ll0) + al0;
    vy = (GRAV + ll1) + al1;
}

// One SwarmEnv._step for the 4 envs of the block, state in LDS (agents) / registers (own locust).
// Agent lanes (tid < 40) carry (actx, acty) = action BEFORE wind and (anx, any) raw noise; act32: the action came from a
// float32 row and its wind / dt arithmetic is float32 (x_update_f32v).
// On return L.p holds the new positions of all 90 points, L.rew[el] the reward; ends on a barrier.
template <int MATH>
__device__ __forceinline__ void block_step(SwarmLds &L, int tid, int el, int j, double &xj, double &yj, double actx,
                                           double acty, double anx, double any, double pnx, double pny, bool act32 = false,
                                           bool wind = true) {
    if (tid < SWARM_EPB * N_AGENTS) {
        int ea = tid / N_AGENTS, a = tid - ea * N_AGENTS;
        double2 q = L.p[ea][N_LOCUSTS + a];
        // wind: `if add_wind: v_action[:, 0] += WIND_SPEED` (multiagent.py:35-36); the locusts' U in v_calculate does not depend on it
        if (act32) x_update_f32v(q.x, q.y, wind ? (float)actx + 1.0f : (float)actx, (float)acty, anx, any);
        else x_update(q.x, q.y, wind ? actx + WIND : actx, acty, anx, any);
        L.p[ea][N_LOCUSTS + a] = q;
    }
    L.p[el][j] = make_double2(xj, yj);
    __syncthreads();
    double vx, vy;
    locust_velocity<MATH>(L.p[el], xj, yj, vx, vy);
    L.en[el][j] = vx * vx + vy * vy;
    x_update(xj, yj, vx, vy, pnx, pny);
    __syncthreads();
    L.p[el][j] = make_double2(xj, yj);
    if (j == 0) {   // energy = mean_j |v_j|^2, numpy pairwise order for n=80 (multiagent.py:114)
        const double *e = L.en[el];
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = e[k];
        for (int i = 8; i < N_LOCUSTS; i += 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] += e[i + k];
        }
        double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        L.rew[el] = -(s / (double)N_LOCUSTS);
    }
    __syncthreads();
}

// ---- the compact observation: SwarmStateProcessor.process_state (state_processors.py:29-42) from positions in LDS / registers
// (swarm.hip's step, reset and observe kernels; net_field_eval.inc's whole-episode kernel)

// searchsorted(edges, v, 'right') for edges = linspace(lo, hi, G+1) as numpy builds them:
// edge(k) = k*step + lo (two roundings), edge(G) = hi exactly (state_processors.py:31 via histogramdd).
__device__ __forceinline__ double edge_at(int k, double lo, double hi, double step, int G) {
    return (k >= G) ? hi : ((double)k * step + lo);
}
__device__ __forceinline__ int count_edges_le(double v, double lo, double hi, double step, int G) {
    if (!(v >= lo)) return 0;        // below the first edge (or NaN)
    if (v >= hi) return G + 1;
    double gf = floor((v - lo) / step);
    int g = (gf > (double)G) ? G : (int)gf;   // guess: index of the last edge <= v
    if (g < 0) g = 0;
    for (int it = 0; it < 4 && g < G && edge_at(g + 1, lo, hi, step, G) <= v; ++it) ++g;
    for (int it = 0; it < 4 && g > 0 && edge_at(g, lo, hi, step, G) > v; ++it) --g;
    return g + 1;
}

// np.mean(vstack([x, xa]), axis=0)[0] of an env's 90 points: sequential row-by-row sum, then /90
__device__ __forceinline__ double swarm_mean_x(const double2 *pts) {
    double s = pts[0].x;
    for (int i = 1; i < N_POINTS; ++i) s += pts[i].x;
    return s / (double)N_POINTS;
}

// The bin pair of one point as bx | by << 8, 0xFFFF outside the box; cx / cy: the counts of edges <= the point's coordinates.
__device__ __forceinline__ uint16_t swarm_point_bin(double px, double py, double meanx, int G, int &cx, int &cy) {
    const double ylo = 0.0, yhi = 6.0;                 // [0, 2*HEIGHT]  (state_processors.py:27)
    const double ystep = (yhi - ylo) / (double)G;
    double lo = meanx - 1.5, hi = meanx + 1.5;         // WIDTH/2 (state_processors.py:27)
    double step = (hi - lo) / (double)G;
    cx = count_edges_le(px, lo, hi, step, G);
    cy = count_edges_le(py, ylo, yhi, ystep, G);
    int bx = (px == hi) ? G - 1 : cx - 1;              // histogramdd: a value on the last edge joins the last bin
    int by = (py == yhi) ? G - 1 : cy - 1;
    bool in = bx >= 0 && bx < G && by >= 0 && by < G;
    return in ? (uint16_t)(bx | (by << 8)) : (uint16_t)0xFFFF;
}

// an agent's position pair: np.digitize == count of edges <= v, clamped to G-1 (state_processors.py:35-40, quirk Q2)
__device__ __forceinline__ uint16_t swarm_point_pos(int cx, int cy, int G) {
    int px = cx >= G ? G - 1 : cx;
    int py = cy >= G ? G - 1 : cy;
    return (uint16_t)(px | (py << 8));
}

// Host side of the whole-episode kernels (swarm_replay.hip, swarm_rules.hip, swarm_plan.hip).
// launch(M) with decltype(M)::value the handle's arithmetic, as launch_swarm (swarm.hip) picks it for the step
template <typename F>
static void swarm_math_dispatch(const grl_handle *h, F &&launch) {
    if (h->cfg.flags & GRL_F_SWARM_FAST_MATH) launch(std::integral_constant<int, MATH_FAST>{});
    else if (h->sw.ref_div) launch(std::integral_constant<int, MATH_REFDIV>{});
    else launch(std::integral_constant<int, MATH_EXACT>{});
}

// the start state both kernels' parameter structs begin with
template <typename P>
static void swarm_start_state(const grl_handle *h, P &p) {
    p.x = h->sw.x; p.xa = h->sw.xa; p.pnoise = h->sw.pnoise; p.anoise = h->sw.anoise; p.elapsed = h->elapsed;
}

// A call's own copy of the positions and its own clock (the planners): the copy starts as the handle's positions, the clock at zero.
static int swarm_start_copy(grl_handle *h, double *x, double *xa, int32_t *length, uint8_t *finished) {
    const size_t E = (size_t)h->E;
    GRL_HIP(h, hipMemcpyAsync(x, h->sw.x, E * N_LOCUSTS * 2 * 8, hipMemcpyDeviceToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(xa, h->sw.xa, E * N_AGENTS * 2 * 8, hipMemcpyDeviceToDevice, h->stream));
    GRL_HIP(h, hipMemsetAsync(length, 0, E * 4, h->stream));
    GRL_HIP(h, hipMemsetAsync(finished, 0, E, h->stream));
    return GRL_OK;
}

// The kept actions (act rows; 0: none kept) and the traced env's positions (trace rows; 0: no env traced) read as zero past a unit's length.
static int swarm_zero_kept(grl_handle *h, double *actions, size_t act, double *trace_x, double *trace_xa, size_t trace) {
    if (act) GRL_HIP(h, hipMemsetAsync(actions, 0, act * N_AGENTS * 2 * 8, h->stream));
    if (trace) {
        GRL_HIP(h, hipMemsetAsync(trace_x, 0, trace * N_LOCUSTS * 2 * 8, h->stream));
        GRL_HIP(h, hipMemsetAsync(trace_xa, 0, trace * N_AGENTS * 2 * 8, h->stream));
    }
    return GRL_OK;
}

}  // namespace grl
