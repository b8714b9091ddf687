// The statistics of a pair, once for the whole-episode launches that keep them (solow_sweep, trade_sweep, trade_foresight,
// ticker_sweep, ticker_foresight and the play kernel of solow_dp): what a kernel accumulates per step reward, and the six per-pair
// output buffers it ends in.  Included by common.h, whose *State structs embed PairStats; the host half is in episode_host.h.
#pragma once
#include <hip/hip_runtime.h>

namespace grl {

// sum, sum of squares (float64) and extremes (float32) of the step rewards of one pair, in registers
struct RewardStats {
    double tot = 0.0, ssq = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    __device__ __forceinline__ void add(float rew) {
        tot += (double)rew;
        ssq += (double)rew * (double)rew;
        mn = fminf(mn, rew);
        mx = fmaxf(mx, rew);
    }
};

// the six per-pair outputs every such launch has: "total", "sum_sq", "min", "max", "length", "finished"
struct PairStats {
    double *total, *sum_sq;
    float *mn, *mx;
    int32_t *length;
    uint8_t *finished;
    __device__ __forceinline__ void store(size_t o, const RewardStats &s, int len, bool fin) const {
        total[o] = s.tot; sum_sq[o] = s.ssq; mn[o] = s.mn; mx[o] = s.mx;
        length[o] = len; finished[o] = fin ? 1 : 0;
    }
};

}  // namespace grl
