// The look-up of the attainable optimum's policy table (include/goldsrl_tradedp.h), ONE copy for its two readers: the play of the
// table (trade_dp.hip: trade_dp_play_kernel, and the solve's own interpolation) and the grid trader's teacher (net_gridtrade.hip:
// gt_teach_forward_kernel).  Everything is float64 and unfused, one IEEE operation per statement, so that both readers give the
// same bits from the same account.
#pragma once

#include "../../include/goldsrl_tradedp.h"

namespace grl {

// position on a uniform axis of n points, `pos` in units of the step from point 0, clamped to the axis: the lower neighbour and
// the share of the upper one.  A NaN lands on point 0, so the index is always inside the table.
struct TdpCoord { int i; double f; };
__device__ __forceinline__ TdpCoord tdp_coord(double pos, int n) {
    pos = fmin(fmax(pos, 0.0), (double)(n - 1));
    int i = (int)pos;
    if (i > n - 2) i = n - 2;
    return TdpCoord{i, pos - (double)i};
}

__device__ __forceinline__ double tdp_lerp(double f, double lo, double hi) {
    const double w = 1.0 - f;
    const double a = w * lo;
    const double b = f * hi;
    return a + b;
}

// the price half of the 2n-linear blend of component `comp` of one table row at share node s: axes x_0 (, x_1), the last innermost
template <int N>
__device__ __forceinline__ double tdp_blend_x(const float *__restrict__ row, size_t s, int NX, int nx, TdpCoord x0, TdpCoord x1, int comp) {
    const float *b = row + s * NX * N + comp;
    if constexpr (N == 1) {
        return tdp_lerp(x0.f, (double)b[x0.i], (double)b[x0.i + 1]);
    } else {
        const float *b0 = b + ((size_t)x0.i * nx + x1.i) * 2;
        const size_t d0 = (size_t)nx * 2;
        const double lo = tdp_lerp(x1.f, (double)b0[0], (double)b0[2]);
        const double hi = tdp_lerp(x1.f, (double)b0[d0], (double)b0[d0 + 2]);
        return tdp_lerp(x0.f, lo, hi);
    }
}

// the whole blend: the share axes u_0 (, u_1) around the price half
template <int N>
__device__ __forceinline__ double tdp_blend(const float *__restrict__ row, int NX, int nx, int nu, TdpCoord u0, TdpCoord u1, TdpCoord x0, TdpCoord x1, int comp) {
    if constexpr (N == 1) {
        return tdp_lerp(u0.f, tdp_blend_x<1>(row, u0.i, NX, nx, x0, x1, comp), tdp_blend_x<1>(row, u0.i + 1, NX, nx, x0, x1, comp));
    } else {
        const size_t s = (size_t)u0.i * nu + u1.i;
        const double lo = tdp_lerp(u1.f, tdp_blend_x<2>(row, s, NX, nx, x0, x1, comp), tdp_blend_x<2>(row, s + 1, NX, nx, x0, x1, comp));
        const double hi = tdp_lerp(u1.f, tdp_blend_x<2>(row, s + nu, NX, nx, x0, x1, comp), tdp_blend_x<2>(row, s + nu + 1, NX, nx, x0, x1, comp));
        return tdp_lerp(u0.f, lo, hi);
    }
}

// what a reader needs of the grid: the axes of the table
struct TdpAxes {
    double um1, x_max, dx;                       // nu - 1; the price axis' end and step (x_max + x_max) / (nx - 1)
    int nu, nx, NX;
    size_t NS;                                   // nu^n * nx^n
};

static inline TdpAxes tdp_axes(const grl_trade_dp_grid &g, int n) {
    const size_t NU = n == 1 ? (size_t)g.nu : (size_t)g.nu * g.nu, NX = n == 1 ? (size_t)g.nx : (size_t)g.nx * g.nx;
    return TdpAxes{(double)(g.nu - 1), g.x_max, (g.x_max + g.x_max) / (double)(g.nx - 1), g.nu, g.nx, (int)NX, NU * NX};
}

// price moves left after a step that begins at `elapsed`: to the TimeLimit, or the table's whole horizon without one
__device__ __forceinline__ int tdp_moves(int max_steps, int elapsed, int horizon) { return max_steps > 0 ? max_steps - elapsed - 1 : horizon; }

// The table's action on the account (cash, q, p) a step begins with, `moves` price moves left after it: 0 when none is left, else
// row min(moves, horizon) - 1 at u_a = q_a p_a / W and x_a = log p_a, the 2n-linear blend rounded once to float32.
// only >= 0: that component alone is blended (the teacher's wave owns one output); the other stays 0.
template <int N>
__device__ __forceinline__ void tdp_lookup(const TdpAxes &A, const float *__restrict__ policy, int horizon, int moves, double cash, const double *q,
                                           const double *p, float *act, int only = -1) {
#pragma unroll
    for (int a = 0; a < 2; ++a) act[a] = 0.f;
    if (moves > 0) {
        const int rw = (moves < horizon ? moves : horizon) - 1;
        const float *row = policy + (size_t)rw * A.NS * N;
        double val[2] = {0.0, 0.0};
        double W = cash;
#pragma unroll
        for (int a = 0; a < N; ++a) { val[a] = q[a] * p[a]; W = W + val[a]; }
        TdpCoord cu[2] = {{0, 0.0}, {0, 0.0}}, cx[2] = {{0, 0.0}, {0, 0.0}};
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double u = val[a] / W;
            cu[a] = tdp_coord(u * A.um1, A.nu);
            const double s = log(p[a]) + A.x_max;
            cx[a] = tdp_coord(s / A.dx, A.nx);
        }
#pragma unroll
        for (int a = 0; a < N; ++a) if (only < 0 || a == only) act[a] = (float)tdp_blend<N>(row, A.NX, A.nx, A.nu, cu[0], cu[1], cx[0], cx[1], a);
    }
}

}  // namespace grl
