// The common-region point filter of one image pair (check_common_points against both masks + apply_homography_to_points of the
// kept destination rows, train_utils.py:350-369): ONE body for balf_common_points_batch (repeat_batch.hip) and
// balf_common_points_index_batch (match_eval.hip), so that the two keep the same rows in the same order with the same bits.
// The mask test is common_mask.h's, the ordered compaction block_ops.h's, the warp homography.h's.
#pragma once
#include "block_ops.h"
#include "common.h"
#include "common_mask.h"
#include "homography.h"
#include "repeat_core.h"

namespace balf {
namespace {

// The work of one workgroup of 256 (all threads call; p = blockIdx.x).  Side 0 keeps the source rows inside mask_src (copied),
// side 1 the destination rows inside mask_dst (warped by h_dst_2_src, score carried).  Kept rows keep their order; rows past
// the kept count are zeroed.  WITH_INDEX: src_index [P,ns_max] / dst_index [P,nd_max] get the original row of each kept row,
// -1 past the kept count.
template <bool WITH_INDEX>
__device__ __forceinline__ void common_points_pair(const double *src, const int *ns, int ns_max, const double *dst, const int *nd,
                                                   int nd_max, const double *h_all, const int *shapes, double *src_out,
                                                   double *dst_out, int *kept, int *valid, int *src_index, int *dst_index,
                                                   int *wcnt /*[4], LDS*/) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const double *h = h_all + 9 * (long)p;
    double m_src[9], m_dst[9];
    const bool inv_ok = common_mask_maps(h, m_src, m_dst);       // (every thread: two closed-form inverses)
    const int hs = shapes[4 * p], ws = shapes[4 * p + 1], hd = shapes[4 * p + 2], wd = shapes[4 * p + 3];
    const bool shape_ok = hs > 0 && ws > 0 && hd > 0 && wd > 0;
    int kept_side[2];
    for (int side = 0; side < 2; ++side) {
        const int n_max = side ? nd_max : ns_max;
        const int n = inv_ok && shape_ok ? clamp_count(side ? nd : ns, p, n_max) : 0;
        const double *in = (side ? dst : src) + (long)p * n_max * 4;
        double *out = (side ? dst_out : src_out) + (long)p * n_max * 4;
        const double *m = side ? m_dst : m_src;
        const int h_out = side ? hd : hs, w_out = side ? wd : ws, h_in = side ? hs : hd, w_in = side ? ws : wd;
        int base = 0;
        for (int r0 = 0; r0 < n; r0 += 256) {
            const int r = r0 + tid;
            double x = 0.0, y = 0.0, rad = 0.0, sc = 0.0;
            bool keep = false;
            if (r < n) {
                x = in[4 * r]; y = in[4 * r + 1]; rad = in[4 * r + 2]; sc = in[4 * r + 3];
                keep = point_in_mask(m, x, y, h_out, w_out, h_in, w_in);
            }
            const int q = compact_slot<256>(keep, wcnt, base);
            if (keep) {
                double *o = out + 4 * (long)q;
                if (side) homography_point(h, x, y, rad, &o[0], &o[1], &o[2]);
                else { o[0] = x; o[1] = y; o[2] = rad; }
                o[3] = sc;
                if constexpr (WITH_INDEX) (side ? dst_index : src_index)[(long)p * n_max + q] = r;
            }
        }
        for (long k = 4 * (long)base + tid; k < 4 * (long)n_max; k += 256) out[k] = 0.0;
        if constexpr (WITH_INDEX) {
            int *index = (side ? dst_index : src_index) + (long)p * n_max;
            for (int k = base + tid; k < n_max; k += 256) index[k] = -1;
        }
        kept_side[side] = base;
    }
    if (tid == 0) {
        kept[2 * p] = kept_side[0];
        kept[2 * p + 1] = kept_side[1];
        valid[p] = kept_side[0] > 0 && kept_side[1] > 0;         // the reference `continue`s otherwise (train_utils.py:355-362)
    }
}

// the limits shared by the batched per-pair calls: 1 <= P <= kMaxPairs, list lengths <= kMaxPoints, ns_max * nd_max < 2^31
inline int check_sizes(int P, int ns_max, int nd_max) {
    if (P <= 0 || P > kMaxPairs || ns_max < 0 || nd_max < 0 || ns_max > kMaxPoints || nd_max > kMaxPoints) return BALF_ERR_ARG;
    if ((long long)ns_max * nd_max > 0x7fffffffLL) return BALF_ERR_SHAPE;
    return BALF_OK;
}

}  // namespace
}  // namespace balf
