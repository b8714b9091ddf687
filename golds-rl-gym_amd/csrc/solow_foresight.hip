// Perfect-foresight ceiling for Solow at any order (C ABI: include/goldsrl_solowforesight.h): the shock path of an episode is fixed
// by the tape the reset drew, so given the path the only state is k, and every env solves its own episode by a one-dimensional
// backward induction and plays the plan.  One kernel, solow_foresight_kernel, one workgroup of four waves per env, three phases:
//   1. Path.  One lane rolls solow_shock_next over the env's tape, the next entry asked for a step ahead, and stores expf(z_t) in
//      the env's column of `ez`: the recursion runs forward, the induction reads it backwards.  Meanwhile the other lanes fill
//      the node tables in LDS (k_i^0.33 and (1 - delta) k_i: pow once per node, not once per stage) and clear what lies past L_e.
//   2. Induction.  V double-buffered in LDS; per stage wave w takes the nodes w, w + 4, .., its lanes the rates, and the wave
//      arg-max of solow_dp_stage_kernel finishes a node.  One barrier per stage: V and the row of decision bytes are each kept
//      twice, so a wave may start stage t - 1 while the others still copy stage t's row to global memory, nk coalesced bytes.  The
//      next stage's ez is asked for before the stage is computed.  The stages of an env are a dependent chain of L_e barriers;
//      nothing crosses workgroups, and the launch is as wide as there are envs.
//   3. Play.  Wave 0 plays while the env's decisions are still in L2.  The state is wave-uniform (every lane computes the same
//      step, the wave's time is one lane's); lane l holds bytes l, l + 64, .. of the decision row, so the two bracketing nodes'
//      decisions are one uniform register choice and one cross-lane read each, and the row of step t + 1 is loaded while step t is
//      computed.  Statistics are RewardStats / PairStats of episode_dev.h, the step is solow_capital_step.
// LDS at any nk: 2 x 8 KB of V, 2 x 8 KB of node tables, 2 KB of decision rows.  Everything in phases 1 and 2 but the path is
// float64 and unfused, so that only log / pow / exp differ from the numpy restatement (tests/_solow_foresight_oracle.py).  The
// handle's state is read only; the error counter is the call's own.
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"
#include "dp_axis.h"

namespace grl {

constexpr int FS_NK = GRL_SOLOW_FORESIGHT_MAX_NK;
constexpr int FS_SLOTS = FS_NK / 64;                           // decision bytes a lane of the playing wave holds
static_assert(GRL_SOLOW_FORESIGHT_MAX_NS <= 256, "a decision is one byte");

// the grid and what the host derives from it once; envs env0 .. env0 + gridDim.x - 1 of the handle are this launch's
struct ForesightArgs {
    double lk_lo, dlk, s_lo, ds, delta, k_lo, k_hi;
    int nk, ns, T, trace_steps, env0;
};

struct ForesightOut {
    PairStats stats;
    double *value;
    int32_t *clamped;
    float *ez;                                                  // (T, E)
    uint8_t *dec;                                               // (envs of the launch, T, nk)
    float *trace_a, *trace_r, *trace_k;
};

// lane l's share of a decision row: bytes l, l + 64, ..
__device__ __forceinline__ void fs_load_row(const uint8_t *row, int nk, int lane, uint32_t (&b)[FS_SLOTS]) {
#pragma unroll
    for (int j = 0; j < FS_SLOTS; ++j) {
        const int i = j * 64 + lane;
        b[j] = (j * 64 < nk && i < nk) ? row[i] : 0u;
    }
}

// byte i (wave-uniform) of the row the wave holds
__device__ __forceinline__ int fs_row_byte(const uint32_t (&b)[FS_SLOTS], int i) {
    const int slot = i >> 6;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < FS_SLOTS; ++j) if (j == slot) v = b[j];
    return __shfl((int)v, i & 63);
}

__global__ __launch_bounds__(256) void solow_foresight_kernel(SolowParams S, SolowShockCoef C, ForesightArgs A, ForesightOut O) {
    __shared__ double v[2][FS_NK];
    __shared__ double kp[FS_NK], kd[FS_NK];
    __shared__ uint8_t dec[2][FS_NK];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int env = A.env0 + blockIdx.x;
    if (env >= S.E) return;                                     // block-uniform
    const size_t E = S.E;
    const int nk = A.nk;
    const int pos0 = S.tape_pos[env], el0 = S.elapsed[env];
    int want = A.T;                                             // the steps the two limits allow; the tape may hold fewer
    if (S.max_steps > 0) {
        const int left = S.max_steps - el0 > 1 ? S.max_steps - el0 : 1;
        want = left < want ? left : want;
    }
    const int tape_left = pos0 >= 0 ? pos0 + 1 : 0;
    const int L = tape_left < want ? tape_left : want;
    float *ez_col = O.ez + env;                                 // stride E
    uint8_t *rows = O.dec + (size_t)blockIdx.x * A.T * nk;

    // ------------------------------------------------------------------------------------------ 1. the path and the node tables
    for (int i = tid; i < nk; i += 256) {
        const double k = exp(A.lk_lo + (double)i * A.dlk);
        kp[i] = pow(k, 0.33);
        kd[i] = (1.0 - A.delta) * k;
        v[0][i] = 0.0;
        v[1][i] = 0.0;
    }
    if (tid == 0) {
        float zr[8], er[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            zr[j] = j >= 8 - C.P ? S.z[(size_t)(j - (8 - C.P)) * E + env] : 0.f;
            er[j] = j >= 8 - C.Q ? S.e[(size_t)(j - (8 - C.Q)) * E + env] : 0.f;
        }
        float e_t = pos0 >= 0 ? S.tape[(size_t)pos0 * E + env] : 0.f;
        for (int t = 0; t < L; ++t) {
            const int pos = pos0 - t;                           // >= 0: t < L <= pos0 + 1
            const float e_next = pos >= 1 ? S.tape[(size_t)(pos - 1) * E + env] : 0.f;     // next step's shock, asked for a step ahead
            ez_col[(size_t)t * E] = expf(zr[7]);
            solow_shock_next(C, zr, er, e_t);
            e_t = e_next;
        }
    }
    for (int t = L + tid; t < A.T; t += 256) ez_col[(size_t)t * E] = 0.f;
    for (size_t o = (size_t)L * nk + tid; o < (size_t)A.T * nk; o += 256) rows[o] = 0;
    __syncthreads();

    // ------------------------------------------------------------------------------------------ 2. the induction
    float ez_f = L > 0 ? ez_col[(size_t)(L - 1) * E] : 0.f;
    for (int t = L - 1; t >= 0; --t) {
        const double ez = (double)ez_f;
        if (t > 0) ez_f = ez_col[(size_t)(t - 1) * E];          // the next stage's, in flight while this one is computed
        const double *vn = v[(t + 1) & 1];
        double *vc = v[t & 1];
        uint8_t *dc = dec[t & 1];
        for (int i = wave; i < nk; i += 4) {                    // wave-uniform node
            const double y = ez * kp[i], kept = kd[i];
            double best = -__builtin_huge_val();
            int best_a = 0x7fffffff;
            for (int a = lane; a < A.ns; a += 64) {
                const double s = fmax(1e-3, A.s_lo + (double)a * A.ds);
                const double r = log((1.0 - s) * y + 1e-4);
                const DpCoord ck = dp_coord(log(kept + s * y), A.lk_lo, A.dlk, nk);
                const double q = r + ((1.0 - ck.f) * vn[ck.i] + ck.f * vn[ck.i + 1]);
                if (q > best) { best = q; best_a = a; }        // ascending a: the lowest index keeps a tie
            }
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) {
                const double oq = __shfl_xor(best, x);
                const int oa = __shfl_xor(best_a, x);
                if (oq > best || (oq == best && oa < best_a)) { best = oq; best_a = oa; }
            }
            if (lane == 0) {
                vc[i] = best;
                dc[i] = (uint8_t)best_a;
            }
        }
        __syncthreads();                                        // the stage's only barrier: V_t and its row are whole
        for (int i = tid; i < nk; i += 256) rows[(size_t)t * nk + i] = dc[i];
    }
    __syncthreads();                                            // row 0 is in global memory
    if (wave != 0) return;

    // ------------------------------------------------------------------------------------------ 3. the play, wave-uniform
    float k = S.k[env];
    const DpCoord c0 = dp_coord(log((double)k), A.lk_lo, A.dlk, nk);
    const double value = (1.0 - c0.f) * v[0][c0.i] + c0.f * v[0][c0.i + 1];      // stage 0 wrote v[0]; zeros when L == 0
    RewardStats rs;
    int clamped = 0;
    uint32_t cur[FS_SLOTS], nxt[FS_SLOTS];
    fs_load_row(rows, L > 0 ? nk : 0, lane, cur);
    float ez_cur = L > 0 ? ez_col[0] : 0.f, ez_nxt = 0.f;
    for (int t = 0; t < L; ++t) {
        const bool more = t + 1 < L;
        fs_load_row(rows + (size_t)(more ? t + 1 : t) * nk, more ? nk : 0, lane, nxt);     // step t + 1's row, in flight during step t
        if (more) ez_nxt = ez_col[(size_t)(t + 1) * E];
        const double kk = (double)k;
        if (kk < A.k_lo || kk > A.k_hi) ++clamped;
        const DpCoord ck = dp_coord(log(kk), A.lk_lo, A.dlk, nk);
        const int i = __builtin_amdgcn_readfirstlane(ck.i);
        const double s0 = A.s_lo + (double)fs_row_byte(cur, i) * A.ds, s1 = A.s_lo + (double)fs_row_byte(cur, i + 1) * A.ds;
        const float s = (float)((1.0 - ck.f) * s0 + ck.f * s1);
        const float rew = solow_capital_step(ez_cur, S.delta, s, k);
        rs.add(rew);
        if (t < A.trace_steps && lane == 0) {
            const size_t o = (size_t)t * E + env;
            O.trace_a[o] = s; O.trace_r[o] = rew; O.trace_k[o] = k;
        }
#pragma unroll
        for (int j = 0; j < FS_SLOTS; ++j) cur[j] = nxt[j];
        ez_cur = ez_nxt;
    }
    for (int t = L + lane; t < A.trace_steps; t += 64) {        // rows are defined up to the env's length; the rest reads as zero
        const size_t o = (size_t)t * E + env;
        O.trace_a[o] = 0.f; O.trace_r[o] = 0.f; O.trace_k[o] = 0.f;
    }
    if (lane == 0) {
        if (L < want) atomicAdd(S.err_flag, 1);                 // reference: IndexError, pop from empty list
        O.stats.store(env, rs, L, S.max_steps > 0 && el0 + L >= S.max_steps);
        O.value[env] = value;
        O.clamped[env] = clamped;
    }
}

// the cap on the decision table: the header's, or a lower one from the environment (the several-launch path at test sizes)
static size_t foresight_table_cap() {
    const char *v = getenv("GRL_SOLOW_FORESIGHT_TABLE_BYTES");
    if (v && *v) {
        char *end = nullptr;
        const unsigned long long n = strtoull(v, &end, 10);
        if (end && *end == 0 && n >= 1 && n < GRL_SOLOW_FORESIGHT_MAX_TABLE_BYTES) return (size_t)n;
    }
    return GRL_SOLOW_FORESIGHT_MAX_TABLE_BYTES;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_solow_foresight(grl_handle *h, const grl_solow_foresight_grid *grid, int32_t max_steps, int32_t trace_steps) {
    const char *fn = "grl_solow_foresight";
    const std::string f(fn);
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SOLOW, "Solow", grid != nullptr)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    if (trace_steps < 0 || trace_steps > max_steps) return fail(h, GRL_E_INVALID, f + ": trace_steps must be in 0..max_steps");
    const grl_solow_foresight_grid &g = *grid;
    if (g.nk < 2 || g.nk > GRL_SOLOW_FORESIGHT_MAX_NK || g.ns < 2 || g.ns > GRL_SOLOW_FORESIGHT_MAX_NS)
        return fail(h, GRL_E_INVALID, f + ": needs 2 <= nk <= " + std::to_string(GRL_SOLOW_FORESIGHT_MAX_NK) + " and 2 <= ns <= " +
                                          std::to_string(GRL_SOLOW_FORESIGHT_MAX_NS));
    if (!(g.k_lo > 0.0) || !(g.k_hi > g.k_lo) || !std::isfinite(g.k_hi)) return fail(h, GRL_E_INVALID, f + ": needs 0 < k_lo < k_hi");
    if (!(g.s_lo >= 0.0) || !(g.s_hi > g.s_lo) || !(g.s_hi <= 1.0)) return fail(h, GRL_E_INVALID, f + ": needs 0 <= s_lo < s_hi <= 1");
    if ((rc = episode_check_idle(h, fn))) return rc;
    const size_t cap = foresight_table_cap(), row = (size_t)max_steps * g.nk;
    if (row > cap)
        return fail(h, GRL_E_SIZE, f + ": one env's decision table (max_steps * nk bytes) would exceed " + std::to_string(cap) + " bytes");
    hipSetDevice(h->cfg.device_id);
    SolowForesightState &d = h->sfs;
    d.played = 0;
    const size_t envs = h->E, chunk = std::min(envs, cap / row), trace = (size_t)trace_steps * envs;
    if ((!d.err && (rc = grow(h, &d.err, 1))) ||
        (rc = episode_reserve(h, d.cap_envs, envs, {buf(d.value), buf(d.clamped)}, &d.stats)) ||
        (rc = episode_reserve(h, d.cap_path, (size_t)max_steps * envs, {buf(d.ez)})) ||
        (rc = episode_reserve(h, d.cap_dec, chunk * row, {buf(d.decisions)})) ||
        (rc = episode_reserve(h, d.cap_trace, trace, {buf(d.trace_a), buf(d.trace_r), buf(d.trace_k)})))
        return rc;
    GRL_HIP(h, hipMemsetAsync(d.err, 0, 4, h->stream));
    SolowParams S = solow_params(h);
    S.err_flag = d.err;
    const SolowShockCoef C = solow_shock_coef(S);
    ForesightArgs A{};
    A.lk_lo = log(g.k_lo);
    A.dlk = (log(g.k_hi) - A.lk_lo) / (double)(g.nk - 1);
    A.s_lo = g.s_lo;
    A.ds = (g.s_hi - g.s_lo) / (double)(g.ns - 1);
    A.delta = h->cfg.solow_delta;
    A.k_lo = g.k_lo; A.k_hi = g.k_hi;
    A.nk = g.nk; A.ns = g.ns; A.T = max_steps; A.trace_steps = trace_steps;
    ForesightOut O{};
    O.stats = d.stats; O.value = d.value; O.clamped = d.clamped; O.ez = d.ez; O.dec = d.decisions;
    O.trace_a = d.trace_a; O.trace_r = d.trace_r; O.trace_k = d.trace_k;
    int launches = 0;
    rc = episode_launch(h, [&] {
        for (size_t e0 = 0; e0 < envs; e0 += chunk, ++launches) {      // the same table, launch after launch: the stream orders them
            A.env0 = (int)e0;
            hipLaunchKernelGGL(solow_foresight_kernel, dim3((unsigned)std::min(chunk, envs - e0)), dim3(256), 0, h->stream, S, C, A, O);
        }
    });
    if (rc) return rc;
    d.grid = g; d.played = h->E; d.max_steps = max_steps; d.trace_steps = trace_steps; d.launches = launches;
    return GRL_OK;
}

int grl_solow_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowForesightState &d = h->sfs;
    const size_t envs = h->E, T = (size_t)d.max_steps, trace = (size_t)d.trace_steps * envs;
    const char *untraced = d.trace_steps == 0 ? "the last call kept no trace (trace_steps was 0)" : nullptr;
    const char *chunked = d.launches > 1 ? "the decision table was capped and the call took several launches: it holds the last launch's envs only" : nullptr;
    const EpisodeOut outs[] = {
        {"value", d.value, envs * 8}, {"clamped", d.clamped, envs * 4}, {"ez", d.ez, T * envs * 4},
        {"decisions", d.decisions, envs * T * (size_t)d.grid.nk, chunked},
        {"actions", d.trace_a, trace * 4, untraced}, {"rewards", d.trace_r, trace * 4, untraced}, {"k", d.trace_k, trace * 4, untraced}};
    return episode_read(h, "grl_solow_foresight_read", GRL_ENV_SOLOW, "Solow", d.played != 0, "grl_solow_foresight", outs, d.err, which, host, bytes,
                        &d.stats, envs);
}

}  // extern "C"
