// create_common_region_masks (balf/benchmark_test/geometry_tools.py:7-26), one pixel at a time: shared by the dense masks
// (balf_common_region_masks, repeat.hip) and the batched point filters (balf_common_points_batch, repeat_batch.hip;
// balf_common_points_index_batch, match_eval.hip) so that they cannot drift.  The reference warps an all-ones image whose 15-pixel frame is zeroed with cv2.warpPerspective
// (default flags: bilinear, constant-zero border), thresholds at 0.75 and zeroes the frame of the result.  Restated here from
// OpenCV's algorithm: the output pixel (x, y) samples the input at M^-1 (x, y, 1), the source coordinates are rounded to
// 1/32 pixel (INTER_TAB_SIZE = 32, round half to even), the four bilinear weights are the exact products of those 5-bit
// fractions.  Parity with cv2 itself is UNPINNED (checked against the oracle's restatement of the same algorithm only).
//
// fp contraction is OFF in every function here: every product and sum below is an individually rounded fp64 operation in source
// order, so that the CPU oracle (NumPy, no FMA) reproduces the 1/32-pixel rounding bit for bit, and so that invert3 gives the
// same bits on the host and on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace balf {
namespace {

constexpr int kCommonBorder = 15;           // create_common_region_masks' fixed frame (geometry_tools.py:16,22)

__host__ __device__ __forceinline__ double ones_inner(int y, int x, int h, int w, int b) {
    return (y >= b && y < h - b && x >= b && x < w - b) ? 1.0 : 0.0;      // zero outside the image too
}

// The source coordinates of output pixel (x, y) under the inverse map m (row-major, homogeneous), rounded to 1/32 pixel as
// cv2.warpPerspective does: *sx, *sy the integer tap (floor), *fx, *fy the 5-bit fractions (0..31).  ONE definition, shared
// by the masks below and by the 8-bit image warp (pair_synth.hip), so that the two sample the same coordinates.
__device__ __forceinline__ void warp_source_q5(const double *m, int y, int x, int *sx, int *sy, int *fx, int *fy) {
#pragma clang fp contract(off)
    const double X0 = m[0] * x + m[1] * y + m[2];
    const double Y0 = m[3] * x + m[4] * y + m[5];
    double W = m[6] * x + m[7] * y + m[8];
    W = W != 0.0 ? 32.0 / W : 0.0;
    const double qx = fmax(-2147483648.0, fmin(2147483647.0, X0 * W));
    const double qy = fmax(-2147483648.0, fmin(2147483647.0, Y0 * W));
    const long long X = llrint(qx), Y = llrint(qy);                         // round half to even, like cvRound
    *sx = (int)(X >> 5);
    *sy = (int)(Y >> 5);
    *fx = (int)(X & 31);
    *fy = (int)(Y & 31);
}

// m: the inverse map, row-major (output pixel -> input coordinates, homogeneous); the mask is h_out x w_out, the all-ones
// image being warped h_in x w_in, both with a zeroed `border` frame
__device__ __forceinline__ double common_mask_pixel(const double *m, int y, int x, int h_out, int w_out, int h_in, int w_in,
                                                    int border) {
#pragma clang fp contract(off)
    double v = 0.0;
    if (y >= border && y < h_out - border && x >= border && x < w_out - border) {
        int sx, sy, fx, fy;
        warp_source_q5(m, y, x, &sx, &sy, &fx, &fy);
        const double ax = (double)fx * (1.0 / 32.0), ay = (double)fy * (1.0 / 32.0);
        const double s = ones_inner(sy, sx, h_in, w_in, border) * ((1.0 - ax) * (1.0 - ay)) +
                         ones_inner(sy, sx + 1, h_in, w_in, border) * (ax * (1.0 - ay)) +
                         ones_inner(sy + 1, sx, h_in, w_in, border) * ((1.0 - ax) * ay) +
                         ones_inner(sy + 1, sx + 1, h_in, w_in, border) * (ax * ay);
        v = s >= 0.75 ? 1.0 : 0.0;
    }
    return v;
}

// check_common_points (repeatability_tools.py:8-13) of one point against the mask of h_out x w_out: mask[round(y) - 1,
// round(x) - 1] with NumPy's indexing (round half to even; -k wraps to row h_out - k).  An index NumPy would reject is
// dropped here (the reference raises IndexError).  ONE definition for every batched point filter (common_points.h).
__device__ __forceinline__ bool point_in_mask(const double *m, double x, double y, int h_out, int w_out, int h_in, int w_in) {
    const double ry = rint(y) - 1.0, rx = rint(x) - 1.0;
    if (!(ry >= -(double)h_out && ry < (double)h_out && rx >= -(double)w_out && rx < (double)w_out)) return false;
    int iy = (int)ry, ix = (int)rx;
    if (iy < 0) iy += h_out;
    if (ix < 0) ix += w_out;
    return common_mask_pixel(m, iy, ix, h_out, w_out, h_in, w_in, kCommonBorder) != 0.0;
}

// closed-form 3x3 inverse (adjugate / determinant), the form OpenCV's cv::invert takes for n <= 3
__host__ __device__ __forceinline__ bool invert3(const double *m, double *o) {
#pragma clang fp contract(off)
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    if (det == 0.0) return false;
    const double r = 1.0 / det;
    o[0] = A * r; o[1] = -(b * i - c * h) * r; o[2] = (b * f - c * e) * r;
    o[3] = B * r; o[4] = (a * i - c * g) * r;  o[5] = -(a * f - c * d) * r;
    o[6] = C * r; o[7] = -(a * h - b * g) * r; o[8] = (a * e - b * d) * r;
    return true;
}

// The two inverse maps of one pair, in balf_common_region_masks' order of operations:
//   mask_src = warp(ones_dst, M = h_dst_2_src): samples ones_dst at M^-1 (x, y, 1)
//   mask_dst = warp(ones_src, M = inv(h_dst_2_src) / its [2,2]): samples ones_src at M^-1 = a multiple of h_dst_2_src
__host__ __device__ __forceinline__ bool common_mask_maps(const double *h_dst_2_src, double *m_src, double *m_dst) {
#pragma clang fp contract(off)
    double inv_h[9];
    if (!invert3(h_dst_2_src, m_src)) return false;
    for (int k = 0; k < 9; ++k) inv_h[k] = m_src[k] / m_src[8];            // the matrix the reference hands to cv2 ...
    return invert3(inv_h, m_dst);                                           // ... and cv2 inverts again
}

}  // namespace
}  // namespace balf
