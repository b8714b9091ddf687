// Constant-savings baseline sweep for Solow (reference scripts/constant_solow.py): every (env, rate) pair plays a whole episode
// from the env's current state in ONE launch (C ABI: include/goldsrl_sweep.h).
//
// Mapping: one lane per env, RPL rates per lane.  The shock path z does not depend on the action, so the lane runs the ARMA
// recursion and expf(z) once per step and carries RPL capitals k over it; powf, logf and the float64 sums run per rate.  The work
// is a dependent chain of expf / powf / logf per step, so it is latency bound; RPL independent chains in a lane hide it where
// there are more pairs than the SIMDs hold waves, and below that a wave per rate (RPL = 1, the default) is faster still.
// z[8] and e[8] are registers (right-aligned, flat_env_dev.h:solow_shock_next), nothing is in LDS, no workgroup talks to
// another.  Lanes of a wave are consecutive envs (one 256-B tape segment per wave and step); the four waves of a workgroup hold
// four rate groups of the SAME 64 envs, so three of them find the tape line in L1/L2.
//
// The handle's state is read only: nothing here writes k, z, e, tape_pos, elapsed, the outputs or the episode records, and the
// error counter is the sweep's own.
#include <stdlib.h>

#include "common.h"
#include "rng.h"
#include "flat_env_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_sweep.h"

namespace grl {

struct SweepOut {
    PairStats stats;
    float *trace_r, *trace_k;
};

template <int RPL>
__global__ __launch_bounds__(256) void solow_sweep_kernel(SolowParams S, SolowShockCoef C, const float *__restrict__ rates, int n_rates,
                                                          int max_steps, int trace_env, SweepOut O) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r0 = (blockIdx.y * 4 + wave) * RPL;          // wave-uniform
    if (r0 >= n_rates || env >= S.E) return;
    const size_t E = S.E;

    float rate[RPL], k[RPL];
    RewardStats rs[RPL];
    const float k0 = S.k[env];
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        rate[j] = rates[r0 + j < n_rates ? r0 + j : n_rates - 1];      // a ragged tail replays the last rate and stores nothing
        k[j] = k0;
    }
    float zr[8], er[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        zr[j] = j >= 8 - C.P ? S.z[(size_t)(j - (8 - C.P)) * E + env] : 0.f;
        er[j] = j >= 8 - C.Q ? S.e[(size_t)(j - (8 - C.Q)) * E + env] : 0.f;
    }
    const int pos0 = S.tape_pos[env], el0 = S.elapsed[env];
    const bool trace = env == trace_env;
    int length = 0;
    bool finished = false;
    float e_t = pos0 >= 0 ? S.tape[(size_t)pos0 * E + env] : 0.f;
    for (int t = 0; t < max_steps; ++t) {
        const int pos = pos0 - t;
        if (pos < 0) {                                       // reference: IndexError, pop from empty list
            if (r0 == 0) atomicAdd(S.err_flag, 1);
            break;
        }
        const float e_next = pos >= 1 ? S.tape[(size_t)(pos - 1) * E + env] : 0.f;     // next step's shock, asked for a step ahead
        const float ez = expf(zr[7]);
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const float rew = solow_capital_step(ez, S.delta, rate[j], k[j]);
            rs[j].add(rew);
            if (trace && r0 + j < n_rates) {
                O.trace_r[(size_t)(r0 + j) * max_steps + t] = rew;
                O.trace_k[(size_t)(r0 + j) * max_steps + t] = k[j];
            }
        }
        solow_shock_next(C, zr, er, e_t);
        e_t = e_next;
        length = t + 1;
        if (S.max_steps > 0 && el0 + length >= S.max_steps) { finished = true; break; }
    }
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        if (r0 + j < n_rates) O.stats.store((size_t)(r0 + j) * E + env, rs[j], length, finished);
    }
}

// rates per lane: 1 is the measured best of 1 / 2 / 4 at 20 rates x 1 024 steps for 1 to 8 192 envs (1.08 / 1.09 / 1.87 ms at
// 4 096, profiles/solow_sweep_times.json): the pairs of such a sweep do not fill the SIMDs, so a rate in a wave of its own beats
// a rate sharing a lane; from 32 768 envs on the three are within 5 % of each other.  GRL_SWEEP_RPL picks another for that
// measurement and for the tests.  Every value gives the same bits.
static int sweep_rpl() {
    const char *v = getenv("GRL_SWEEP_RPL");
    if (v && (v[0] == '1' || v[0] == '2' || v[0] == '4') && v[1] == 0) return v[0] - '0';
    return 1;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_solow_sweep(grl_handle *h, const float *rates_host, int32_t n_rates, int32_t max_steps, int32_t trace_env) {
    const char *fn = "grl_solow_sweep";
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_SOLOW, "Solow", rates_host)) || (rc = episode_check_count(h, fn, "n_rates", n_rates, 4096)) ||
        (rc = episode_check_steps(h, fn, max_steps)) || (rc = episode_check_trace_env(h, fn, trace_env)) || (rc = episode_check_idle(h, fn)))
        return rc;
    hipSetDevice(h->cfg.device_id);
    SolowSweepState &w = h->swp;
    w.n_rates = 0;
    const size_t pairs = (size_t)n_rates * h->E, trace = trace_env >= 0 ? (size_t)n_rates * max_steps : 0;
    if ((!w.err && (rc = grow(h, &w.err, 1))) || (rc = episode_reserve(h, w.cap_rates, n_rates, {buf(w.rates)})) ||
        (rc = episode_reserve(h, w.cap_pairs, pairs, {}, &w.stats)) ||
        (rc = episode_reserve(h, w.cap_trace, trace, {buf(w.trace_r), buf(w.trace_k)})))
        return rc;
    GRL_HIP(h, hipMemcpyAsync(w.rates, rates_host, (size_t)n_rates * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemsetAsync(w.err, 0, 4, h->stream));
    if (trace) {     // rows are defined up to the pair's length; the rest reads as zero
        GRL_HIP(h, hipMemsetAsync(w.trace_r, 0, trace * 4, h->stream));
        GRL_HIP(h, hipMemsetAsync(w.trace_k, 0, trace * 4, h->stream));
    }
    SolowParams S = solow_params(h);
    S.err_flag = w.err;
    const SolowShockCoef C = solow_shock_coef(S);
    SweepOut O{};
    O.stats = w.stats; O.trace_r = w.trace_r; O.trace_k = w.trace_k;
    const int rpl = sweep_rpl();
    const int groups = (n_rates + rpl - 1) / rpl;
    const dim3 grid((h->E + 63) / 64, (groups + 3) / 4), block(256);
    rc = episode_launch(h, [&] {
        if (rpl == 1) hipLaunchKernelGGL(solow_sweep_kernel<1>, grid, block, 0, h->stream, S, C, w.rates, n_rates, max_steps, trace_env, O);
        else if (rpl == 2) hipLaunchKernelGGL(solow_sweep_kernel<2>, grid, block, 0, h->stream, S, C, w.rates, n_rates, max_steps, trace_env, O);
        else hipLaunchKernelGGL(solow_sweep_kernel<4>, grid, block, 0, h->stream, S, C, w.rates, n_rates, max_steps, trace_env, O);
    });
    if (rc) return rc;
    w.n_rates = n_rates; w.max_steps = max_steps; w.trace_env = trace_env;
    return GRL_OK;
}

int grl_solow_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const SolowSweepState &w = h->swp;
    const size_t pairs = (size_t)w.n_rates * h->E, trace = (size_t)w.n_rates * w.max_steps;
    const char *untraced = w.trace_env < 0 ? "the last sweep traced no env (trace_env was -1)" : nullptr;
    const EpisodeOut outs[] = {{"trace_rewards", w.trace_r, trace * 4, untraced}, {"trace_k", w.trace_k, trace * 4, untraced}};
    return episode_read(h, "grl_solow_sweep_read", GRL_ENV_SOLOW, "Solow", w.n_rates != 0, "grl_solow_sweep", outs, w.err, which, host, bytes, &w.stats, pairs);
}

}  // extern "C"
