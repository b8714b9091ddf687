// The clamping rule of the Solow inductions' uniform axes (solow_dp.hip, solow_arma_dp.hip): one copy, so the two solvers and
// their plays place a coordinate the same way.
#pragma once

namespace grl {

// position on a uniform axis of n points from lo in steps of `step`, clamped to the axis: the lower neighbour and the share of
// the upper one.  A NaN lands on point 0, so the index is always inside the table.
struct DpCoord { int i; double f; };
__device__ __forceinline__ DpCoord dp_coord(double x, double lo, double step, int n) {
    double u = (x - lo) / step;
    u = fmin(fmax(u, 0.0), (double)(n - 1));
    int i = (int)u;
    if (i > n - 2) i = n - 2;
    return DpCoord{i, u - (double)i};
}

}  // namespace grl
