// The point selection of check_val_repeatability (balf/utils/train_utils.py:205-306) for P image pairs x 2 sides on gfx950,
// stream-ordered, nothing read back.  Per side the reference does
//     nms_map = NMS(prob)                       greedy leg: get_nms_score_map_from_score_map (repeatability_tools.py:82-100)
//                                               window leg: apply_nms (:19-23), no border frame in either
//     masked  = nms_map * mask_of_the_side      create_common_region_masks (geometry_tools.py:7-26)
//     rows    = get_point_coordinates(masked, num_points = K, 'xysr')        (geometry_tools.py:86-125)
// and warps the destination rows with apply_homography_to_points.  The selection is NOT the HSequences one (top-K, then the
// mask): the K-th largest value is taken over the MASKED map, and the rows come out in raster order (argwhere), not by score.
//
//   the NMS survivors come from the existing kernels: the window survivor list of nms_topk.hip, the kept list of nms_fast.hip
//   (asked for with a K that cannot truncate: kept points are more than d apart in Chebyshev distance, so every
//   (d+1) x (d+1) cell holds at most one);
//   val_select_kernel   one workgroup per (pair, side):
//       1. the side's mask at each survivor (common_mask.h: the dense masks never exist); a survivor outside it gets score
//          bits 0 in the list, the survivors inside are counted;
//       2. none inside: threshold 0 -> `masked >= 0` holds everywhere -> the first K raster pixels of the map, score 0;
//          at most K inside: the threshold is the smallest positive value -> exactly the survivors inside;
//          more: MSB-first radix select of the K-th largest score, and if more than K reach it a second select on the flat
//          index keeps the raster-first K (`argwhere(map >= thr)[:K]`);
//       3. the selected (flat index, score) pairs are sorted by flat index in LDS (bitonic) and written as float64 rows
//          (x, y, 1.0, score); destination rows go through homography_point first.  Rows past the count are 0.
//   The reduction, the select and the sort are the shared ones of block_ops.h.
#include "block_ops.h"
#include "common.h"
#include "common_mask.h"
#include "homography.h"

int balf_window_survivors_launch(const float *prob_dev, int B, int H, int W, int nms_size, int2 *surv, int *counts,
                                 hipStream_t st);                                                       // nms_topk.hip

namespace balf {
namespace {

constexpr int kSelThreads = 1024;
constexpr int kGreedyMaxDist = 16;          // balf_greedy_nms' limit

// One side's survivors: either the window list (surv != nullptr: [P, cap] (flat index, score bits)) or the greedy rows
// (idx / score [P, cap]); count [P].  The list lives in the workspace: step 1 clears the score of what the mask drops.
struct ValSide {
    int2 *surv;
    int32_t *idx;
    float *score;
    const int *count;
    long cap;
    int H, W;
    double *out;                            // [P, K, 4]
};

struct ValArgs {
    ValSide side[2];
    const double *h;                        // [P, 9] h_dst_2_src
    int K, npow2;
    int32_t *count_out;                     // [P, 2]
};

__device__ __forceinline__ int2 entry(const ValSide &s, long base, int i) {
    return s.surv ? s.surv[base + i] : make_int2(s.idx[base + i], __float_as_int(s.score[base + i]));
}

// grid (P, 2): blockIdx.y = side (0 source, 1 destination)
__global__ __launch_bounds__(kSelThreads) void val_select_kernel(ValArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);       // [npow2]
    unsigned *s_hist = reinterpret_cast<unsigned *>(keys + a.npow2);               // [256]
    int *s_tmp = reinterpret_cast<int *>(s_hist + 256);                            // [4]
    int *s_cnt = s_tmp + 4;                                                        // [1]
    int *s_red = s_cnt + 1;                                                        // [16]

    const int p = blockIdx.x, sd = blockIdx.y, tid = threadIdx.x;
    const ValSide &s = a.side[sd];
    const ValSide &other = a.side[sd ^ 1];
    const int K = a.K, H = s.H, W = s.W;
    const long base = (long)p * s.cap;
    const double *h = a.h + 9 * (long)p;
    double *out = s.out + (long)p * K * 4;
    const int n = clamp_count(s.count, p, (int)s.cap);          // (cap <= H * W < 2^31)

    // 1. the mask at every survivor
    double m_src[9], m_dst[9];
    const bool inv_ok = common_mask_maps(h, m_src, m_dst);       // (every thread: two closed-form inverses)
    const double *m = sd ? m_dst : m_src;
    int mine = 0;
    for (int i = tid; i < n; i += kSelThreads) {
        const int2 e = entry(s, base, i);
        bool in = inv_ok && e.y > 0 && e.x >= 0 && e.x < H * W;
        if (in) {
            const int y = e.x / W, x = e.x - y * W;
            in = common_mask_pixel(m, y, x, H, W, other.H, other.W, kCommonBorder) != 0.0;
        }
        if (in) ++mine;
        else if (s.surv) s.surv[base + i].y = 0;
        else s.score[base + i] = 0.0f;
    }
    const int n_pos = block_sum<kSelThreads>(mine, s_red);        // (its barriers also order the stores above before step 2)

    if (n_pos == 0) {
        // 2a. no positive value in the masked map: the threshold falls back to 0.0 and `map >= 0` holds everywhere
        // (geometry_tools.py:114-123): the first K pixels of the whole map in raster order, with score 0
        for (int i = tid; i < K; i += kSelThreads) {
            const int y = i / W, x = i - y * W;
            double ox = (double)x, oy = (double)y, orad = 1.0;
            if (sd) homography_point(h, (double)x, (double)y, 1.0, &ox, &oy, &orad);
            out[4 * i] = ox; out[4 * i + 1] = oy; out[4 * i + 2] = orad; out[4 * i + 3] = 0.0;
        }
        if (tid == 0) a.count_out[2 * p + sd] = K;
        return;
    }

    // 2b. score >= thr with flat index <= idx_cut.  n_pos <= K: the threshold is the smallest positive value, i.e. every
    // survivor inside the mask (bits >= 1: positive floats order like their bits)
    unsigned thr = 1u;
    int idx_cut = 0x7fffffff;
    auto each = [&](auto f) {                                    // f(entry) for every list entry of this thread
        for (int i = tid; i < n; i += kSelThreads) f(entry(s, base, i));
    };
    if (n_pos > K) {
        int n_eq, need_eq;
        // (the list is read from memory in every pass: it is short or L2-resident)
        thr = (unsigned)radix_select<32, true, kSelThreads>(
            K, [&](auto count) { each([&](int2 e) { if (e.y > 0) count((unsigned)e.y); }); }, s_hist, s_tmp, &n_eq, &need_eq);
        if (n_eq > need_eq) {                                    // more than K reach the threshold: the raster-first K
            int d0, d1;
            const unsigned t = thr;
            idx_cut = (int)radix_select<32, false, kSelThreads>(
                K, [&](auto count) { each([&](int2 e) { if (e.y > 0 && (unsigned)e.y >= t) count((unsigned)e.x); }); }, s_hist,
                s_tmp, &d0, &d1);
        }
    }

    // 3. raster order: sort the selected (flat index, score bits) by flat index
    if (tid == 0) *s_cnt = 0;
    for (int i = tid; i < a.npow2; i += kSelThreads) keys[i] = ~0ull;
    __syncthreads();
    each([&](int2 e) {
        if (e.y > 0 && (unsigned)e.y >= thr && e.x <= idx_cut) {
            const int q = atomicAdd(s_cnt, 1);
            if (q < a.npow2) keys[q] = ((unsigned long long)(unsigned)e.x << 32) | (unsigned)e.y;
        }
    });
    __syncthreads();
    const int cnt = *s_cnt < K ? *s_cnt : K;                     // (== *s_cnt: the selection holds at most K)
    bitonic_sort<kSelThreads>(keys, a.npow2);
    for (int i = tid; i < K; i += kSelThreads) {
        double ox = 0.0, oy = 0.0, orad = 0.0, osc = 0.0;
        if (i < cnt) {
            const unsigned long long kv = keys[i];
            const int flat = (int)(unsigned)(kv >> 32);
            const int y = flat / W, x = flat - y * W;
            ox = (double)x; oy = (double)y; orad = 1.0;
            osc = (double)__uint_as_float((unsigned)(kv & 0xffffffffull));
            if (sd) homography_point(h, (double)x, (double)y, 1.0, &ox, &oy, &orad);
        }
        out[4 * i] = ox; out[4 * i + 1] = oy; out[4 * i + 2] = orad; out[4 * i + 3] = osc;
    }
    if (tid == 0) a.count_out[2 * p + sd] = cnt;
}

// a bound on what the greedy NMS can keep: one point per (d+1) x (d+1) cell
long greedy_keep_bound(int H, int W, int d) { return (long)balf_ceil_div(H, d + 1) * balf_ceil_div(W, d + 1); }

struct SideWs {
    size_t counts, list, idx, score, nms_ws, nms_ws_bytes, end;
    int kg;
};

// the workspace slice of one side starting at byte `o`
SideWs side_layout(size_t o, int P, int H, int W, int leg, int nms_size) {
    SideWs w{};
    WorkspaceCursor c{nullptr, o};
    w.counts = c.offset((size_t)P * 4);
    if (leg == BALF_VAL_LEG_WINDOW) {
        w.list = c.offset((size_t)P * H * W * sizeof(int2));
    } else {
        w.kg = (int)greedy_keep_bound(H, W, nms_size);
        w.idx = c.offset((size_t)P * w.kg * 4);
        w.score = c.offset((size_t)P * w.kg * 4);
        w.nms_ws_bytes = balf_greedy_nms_workspace_bytes(P, H, W, w.kg);
        w.nms_ws = c.offset(w.nms_ws_bytes);
    }
    w.end = c.used;
    return w;
}

int check_args(int P, int h_src, int w_src, int h_dst, int w_dst, int leg, int nms_size, int K) {
    if (P <= 0 || P > kMaxPairs || h_src <= 0 || w_src <= 0 || h_dst <= 0 || w_dst <= 0 || K <= 0 || K > BALF_MAX_TOPK)
        return BALF_ERR_ARG;
    if (leg == BALF_VAL_LEG_WINDOW) {
        if (nms_size < 1 || nms_size > BALF_MAX_NMS_SIZE) return BALF_ERR_ARG;
    } else if (leg == BALF_VAL_LEG_GREEDY) {
        if (nms_size < 0 || nms_size > kGreedyMaxDist) return BALF_ERR_ARG;
    } else {
        return BALF_ERR_ARG;
    }
    if ((long)h_src * w_src > 0x7fffffffL || (long)h_dst * w_dst > 0x7fffffffL) return BALF_ERR_SHAPE;
    if ((long)K > (long)h_src * w_src || (long)K > (long)h_dst * w_dst) return BALF_ERR_SHAPE;    // the reference: IndexError
    if (leg == BALF_VAL_LEG_GREEDY && (greedy_keep_bound(h_src, w_src, nms_size) > BALF_MAX_TOPK ||
                                       greedy_keep_bound(h_dst, w_dst, nms_size) > BALF_MAX_TOPK))
        return BALF_ERR_SHAPE;
    return BALF_OK;
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_val_points_workspace_bytes(int P, int h_src, int w_src, int h_dst, int w_dst, int leg, int nms_size,
                                                  int K) {
    if (check_args(P, h_src, w_src, h_dst, w_dst, leg, nms_size, K) != BALF_OK) return 0;
    const SideWs s = side_layout(0, P, h_src, w_src, leg, nms_size);
    return side_layout(s.end, P, h_dst, w_dst, leg, nms_size).end;
}

extern "C" int balf_val_points(const float *prob_src_dev, int h_src, int w_src, const float *prob_dst_dev, int h_dst, int w_dst,
                               int P, const double *h_dst_2_src_dev, int leg, float conf_thresh, int nms_size, int K,
                               double *src_pts_dev, double *dst_pts_dev, int32_t *count_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream) {
    if (!prob_src_dev || !prob_dst_dev || !h_dst_2_src_dev || !src_pts_dev || !dst_pts_dev || !count_dev || !workspace_dev)
        return BALF_ERR_ARG;
    int rc = check_args(P, h_src, w_src, h_dst, w_dst, leg, nms_size, K);
    if (rc != BALF_OK) return rc;
    if (leg == BALF_VAL_LEG_GREEDY && !(conf_thresh > 0.0f)) return BALF_ERR_ARG;
    if (workspace_bytes < balf_val_points_workspace_bytes(P, h_src, w_src, h_dst, w_dst, leg, nms_size, K))
        return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_dev);

    ValArgs a{};
    a.h = h_dst_2_src_dev;
    a.K = K;
    a.npow2 = next_pow2(K);
    a.count_out = count_dev;
    size_t o = 0;
    for (int sd = 0; sd < 2; ++sd) {
        const float *prob = sd ? prob_dst_dev : prob_src_dev;
        const int H = sd ? h_dst : h_src, W = sd ? w_dst : w_src;
        const SideWs l = side_layout(o, P, H, W, leg, nms_size);
        o = l.end;
        ValSide &v = a.side[sd];
        v.count = reinterpret_cast<const int *>(ws + l.counts);
        v.H = H;
        v.W = W;
        v.out = sd ? dst_pts_dev : src_pts_dev;
        if (leg == BALF_VAL_LEG_WINDOW) {
            v.surv = reinterpret_cast<int2 *>(ws + l.list);
            v.cap = (long)H * W;
            rc = balf_window_survivors_launch(prob, P, H, W, nms_size, v.surv, reinterpret_cast<int *>(ws + l.counts), st);
        } else {
            v.idx = reinterpret_cast<int32_t *>(ws + l.idx);
            v.score = reinterpret_cast<float *>(ws + l.score);
            v.cap = l.kg;
            rc = balf_greedy_nms(prob, P, H, W, 0, 0, H, W, /*border=*/0, conf_thresh, nms_size, l.kg, /*subpixel_patch=*/0, v.idx,
                                 v.score, nullptr, reinterpret_cast<int32_t *>(ws + l.counts), nullptr, ws + l.nms_ws,
                                 l.nms_ws_bytes, stream);
        }
        if (rc != BALF_OK) return rc;
    }
    const size_t smem = (size_t)a.npow2 * 8 + 256 * 4 + (4 + 1 + 16) * 4;
    if (!balf_allow_dynamic_lds<val_select_kernel>((int)smem)) return BALF_ERR_LAUNCH;
    val_select_kernel<<<dim3(P, 2), kSelThreads, smem, st>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
