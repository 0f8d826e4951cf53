// The matching-score (MMA) leg of the HSequences evaluation on gfx950: what links the filtered point lists to
// the per-image descriptors, and what verifies matches against the ground-truth homography.  P independent pairs,
// stream-ordered; nothing synchronises, nothing is read back, no workspace.
//
//   balf_common_points_index_batch   balf_common_points_batch plus the original row of every kept row
//     common_points_index_kernel     one workgroup per pair: the body of common_points.h with the index outputs
//   balf_match_accuracy_batch        reprojection error of every match, and the matches within each pixel threshold
//     match_accuracy_kernel          one workgroup per pair: a strided walk over the pair's matches, per-thread counts in
//                                    registers, one block_sum (block_ops.h) per threshold
// The thresholds travel as kernel arguments (a struct of 16 doubles by value): no upload, and a captured graph carries them.
// fp contraction is OFF in the error: dx*dx + dy*dy is two rounded products and a rounded sum, as NumPy computes it.
#include "block_ops.h"
#include "common.h"
#include "common_points.h"

namespace balf {
namespace {

constexpr int kMaxThresholds = 16;
constexpr int kMaxMatches = 65536;          // cap <= min(ns_max, nd_max) <= kMaxPoints

struct Thresholds {
    double t[kMaxThresholds];
};

__global__ __launch_bounds__(256) void common_points_index_kernel(const double *src, const int *ns, int ns_max, const double *dst,
                                                                  const int *nd, int nd_max, const double *h_all,
                                                                  const int *shapes, double *src_out, double *dst_out, int *kept,
                                                                  int *valid, int *src_index, int *dst_index) {
    __shared__ int wcnt[4];
    common_points_pair<true>(src, ns, ns_max, dst, nd, nd_max, h_all, shapes, src_out, dst_out, kept, valid, src_index, dst_index,
                             wcnt);
}

// One workgroup of 256 per pair.  Slot k of the pair: err = |S[i] - D'[j]| for (i, j) = match_idx[p, k] when k is below the
// pair's match count and both indices are inside the kept lists, NaN otherwise (a NaN is within no threshold).  Every slot of
// err and of correct is written.
__global__ __launch_bounds__(256) void match_accuracy_kernel(const double *src, int ns_max, const double *dst, int nd_max,
                                                             const int *kept, const int *match_idx, const int *match_count,
                                                             int cap, Thresholds th, int T, double *err, int *correct) {
#pragma clang fp contract(off)
    __shared__ int s_red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int ks = clamp_count(kept, 2 * (long)p, ns_max), kd = clamp_count(kept, 2 * (long)p + 1, nd_max);
    const int m = clamp_count(match_count, p, cap);
    const double *s = src + (long)p * ns_max * 4, *d = dst + (long)p * nd_max * 4;
    const int *mi = match_idx + (long)p * cap * 2;
    double *e_out = err + (long)p * cap;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int cnt[kMaxThresholds];
#pragma unroll
    for (int t = 0; t < kMaxThresholds; ++t) cnt[t] = 0;
    for (int k = tid; k < cap; k += 256) {
        double e = nan;
        if (k < m) {
            const int i = mi[2 * k], j = mi[2 * k + 1];
            if (i >= 0 && i < ks && j >= 0 && j < kd) {
                const double dx = s[4 * (long)i] - d[4 * (long)j], dy = s[4 * (long)i + 1] - d[4 * (long)j + 1];
                e = sqrt(dx * dx + dy * dy);
#pragma unroll
                for (int t = 0; t < kMaxThresholds; ++t) cnt[t] += (t < T && e <= th.t[t]) ? 1 : 0;
            }
        }
        e_out[k] = e;
    }
#pragma unroll
    for (int t = 0; t < kMaxThresholds; ++t) {
        if (t < T) {                                              // (uniform: T is a kernel argument)
            const int c = block_sum<256>(cnt[t], s_red);
            if (tid == 0) correct[(long)p * T + t] = c;
        }
    }
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" int balf_common_points_index_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, const double *dst_dev,
                                              const int32_t *nd_dev, int nd_max, int P, const double *h_dst_2_src_dev,
                                              const int32_t *shapes_dev, double *src_out_dev, double *dst_out_dev,
                                              int32_t *kept_dev, int32_t *valid_dev, int32_t *src_index_dev,
                                              int32_t *dst_index_dev, void *stream) {
    if (!src_dev || !ns_dev || !dst_dev || !nd_dev || !h_dst_2_src_dev || !shapes_dev || !src_out_dev || !dst_out_dev ||
        !kept_dev || !valid_dev || !src_index_dev || !dst_index_dev)
        return BALF_ERR_ARG;
    const int rc = check_sizes(P, ns_max, nd_max);
    if (rc != BALF_OK) return rc;
    common_points_index_kernel<<<P, 256, 0, static_cast<hipStream_t>(stream)>>>(src_dev, ns_dev, ns_max, dst_dev, nd_dev, nd_max,
                                                                                h_dst_2_src_dev, shapes_dev, src_out_dev,
                                                                                dst_out_dev, kept_dev, valid_dev, src_index_dev,
                                                                                dst_index_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_match_accuracy_batch(const double *src_dev, int ns_max, const double *dst_dev, int nd_max,
                                         const int32_t *kept_dev, const int32_t *match_idx_dev, const int32_t *match_count_dev,
                                         int cap, int P, const double *thresholds_host, int T, double *err_dev,
                                         int32_t *correct_dev, void *stream) {
    if (!src_dev || !dst_dev || !kept_dev || !match_idx_dev || !match_count_dev || !thresholds_host || !err_dev || !correct_dev)
        return BALF_ERR_ARG;
    if (T < 1 || T > kMaxThresholds || cap < 1 || cap > kMaxMatches) return BALF_ERR_ARG;
    const int rc = check_sizes(P, ns_max, nd_max);
    if (rc != BALF_OK) return rc;
    Thresholds th{};
    for (int t = 0; t < T; ++t) {
        th.t[t] = thresholds_host[t];
        if (!(th.t[t] >= 0.0) || (t > 0 && !(th.t[t] > th.t[t - 1]))) return BALF_ERR_ARG;      // (NaN fails both)
    }
    match_accuracy_kernel<<<P, 256, 0, static_cast<hipStream_t>(stream)>>>(src_dev, ns_max, dst_dev, nd_max, kept_dev,
                                                                           match_idx_dev, match_count_dev, cap, th, T, err_dev,
                                                                           correct_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
