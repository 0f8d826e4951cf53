// apply_homography_to_points (balf/benchmark_test/geometry_tools.py:43-64) for one point, float64:
// shared by balf_apply_homography (repeat.hip) and the multi-scale merge (multiscale.hip) so that the two agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace balf {

// (x, y, radius) -> the warped point and the radius rescaled by the warp's local affine approximation
__device__ __forceinline__ void homography_point(const double *h, double x, double y, double r, double *ox, double *oy,
                                                 double *orad) {
    constexpr double kEpsF32 = 1.1920928955078125e-07;     // np.finfo(np.float32).eps
    const double den = h[6] * x + h[7] * y + h[8];
    const double nx = h[0] * x + h[1] * y + h[2], ny = h[3] * x + h[4] * y + h[5];
    const double fxdx = h[0] / den - nx * h[6] / (den * den), fxdy = h[1] / den - nx * h[7] / (den * den);
    const double fydx = h[3] / den - ny * h[6] / (den * den), fydy = h[4] / den - ny * h[7] / (den * den);
    const double tmp = r * r + kEpsF32;
    *ox = nx / den;
    *oy = ny / den;
    *orad = sqrt(tmp * fabs(fxdx * fydy - fxdy * fydx));
}

}  // namespace balf
