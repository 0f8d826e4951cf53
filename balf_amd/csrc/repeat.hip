// Repeatability evaluation on gfx950.
//
// Reference: /root/reference/balf/benchmark_test/repeatability_tools.py:379-512 (compute_repeatability,
// intersection_area, union_area) and /root/reference/balf/benchmark_test/geometry_tools.py:43-86
// (apply_homography_to_points, getAff).  The reference walks all Ns x Nd pairs in a Python double loop, fills two
// dense overlap matrices, argsorts each and assigns greedily; callers: train_utils.py:189,257 (validation) and
// datasets/dataset_utils.py:332.
//
// Here nothing dense is stored.  All arithmetic is float64, like the reference's Python floats:
//   rep_count_kernel   one workgroup per source point: circle-overlap of every pair, counts the pairs whose
//                      single-scale / multi-scale overlap reaches 1 - overlap_err, and the "possible match" flag
//   rep_scan_kernel    exclusive scan of the per-row counts
//   rep_fill_kernel    one wave per source point: ordered compaction of the candidate pairs (key = overlap bits,
//                      value = flat index i*Nd + j, written in flat order)
//   rep_sort_kernel    stable LSD radix sort, descending by overlap => equal overlaps stay in flat-index order
//   rep_greedy_kernel  one wave walks the sorted candidates 64 at a time; visited bitmaps in LDS; the error sum is
//                      accumulated in the reference's order
// The candidate count is data dependent and stays on the device.  The overlaps, the sort and the greedy walk are in
// repeat_core.h, shared with the batched entry of repeat_batch.hip; the scan is block_scan_chunk of block_ops.h.
#include "block_ops.h"
#include "common.h"
#include "common_mask.h"
#include "homography.h"
#include "repeat_core.h"

namespace balf {
namespace {

__global__ __launch_bounds__(256) void rep_count_kernel(const double *src, int ns, const double *dst, int nd, RepParams p,
                                                        int *cnt_s, int *cnt_m, int *poss) {
    __shared__ int red[3];
    const int i = blockIdx.x;
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    const double sx = src[3 * i], sy = src[3 * i + 1], sr = src[3 * i + 2];
    int cs = 0, cm = 0, ps = 0;
    for (int j = threadIdx.x; j < nd; j += 256) {
        double s, m; bool po;
        pair_overlaps(sx, sy, sr, dst[3 * j], dst[3 * j + 1], dst[3 * j + 2], p, s, m, po);
        cs += s >= p.thr; cm += m >= p.thr; ps |= po;
    }
    if (cs) atomicAdd(&red[0], cs);
    if (cm) atomicAdd(&red[1], cm);
    if (ps) atomicOr(&red[2], 1);
    __syncthreads();
    if (threadIdx.x == 0) { cnt_s[i] = red[0]; cnt_m[i] = red[1]; poss[i] = red[2]; }
}

// off[i] = sum_{k<i} cnt[k]; totals = {sum cnt_s, sum cnt_m, sum poss}
__global__ __launch_bounds__(1024) void rep_scan_kernel(const int *cnt_s, const int *cnt_m, const int *poss, int ns,
                                                        int *off_s, int *off_m, int *totals, int *poss_out) {
    __shared__ int wsum[3][16];
    __shared__ int base[3];
    const int tid = threadIdx.x;
    if (tid < 3) base[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < ns; i0 += 1024) {
        const int i = i0 + tid;
        const int v[3] = {i < ns ? cnt_s[i] : 0, i < ns ? cnt_m[i] : 0, i < ns ? poss[i] : 0};
        int excl[3];
        block_scan_chunk<int, 3, 1024>(v, excl, wsum, base);
        if (i < ns) { off_s[i] = excl[0]; off_m[i] = excl[1]; }
    }
    if (tid == 0) { totals[0] = base[0]; totals[1] = base[1]; totals[2] = base[2]; *poss_out = base[2]; }
}

__global__ __launch_bounds__(64) void rep_fill_kernel(const double *src, int ns, const double *dst, int nd, RepParams p,
                                                      const int *off_s, const int *off_m, int max_edges,
                                                      unsigned long long *key_s, unsigned *val_s, unsigned long long *key_m,
                                                      unsigned *val_m) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const double sx = src[3 * i], sy = src[3 * i + 1], sr = src[3 * i + 2];
    int ws = off_s[i], wm = off_m[i];
    for (int j0 = 0; j0 < nd; j0 += 64) {
        const int j = j0 + lane;
        double s = 0.0, m = 0.0; bool po;
        if (j < nd) pair_overlaps(sx, sy, sr, dst[3 * j], dst[3 * j + 1], dst[3 * j + 2], p, s, m, po);
        const bool ks = j < nd && s >= p.thr, km = j < nd && m >= p.thr;
        const unsigned long long bs = __ballot(ks), bm = __ballot(km);
        const unsigned long long below = (1ull << lane) - 1ull;
        // a list longer than the caller's max_edges is cut here and reported by rep_greedy_kernel (count -1): the host never
        // learns the length, so nothing waits for it
        if (ks) { const int o = ws + __popcll(bs & below); if (o < max_edges) { key_s[o] = __double_as_longlong(s); val_s[o] = (unsigned)(i * nd + j); } }
        if (km) { const int o = wm + __popcll(bm & below); if (o < max_edges) { key_m[o] = __double_as_longlong(m); val_m[o] = (unsigned)(i * nd + j); } }
        ws += __popcll(bs); wm += __popcll(bm);
    }
}

// out: found[which], err[which], corr[which][k] = (x_pos = dst index, y_pos = src index) in assignment order
// *n_edges_dev > max_edges (the candidate list did not fit the workspace): found = -1, no correspondences
__global__ __launch_bounds__(64) void rep_greedy_kernel(const unsigned long long *keys, const unsigned *vals, const int *n_edges_dev,
                                                        int max_edges, int nd, int *found_out, double *err_out, int *corr, int cap) {
    __shared__ unsigned vis_x[kMaxPoints / 32], vis_y[kMaxPoints / 32];
    const int lane = threadIdx.x;
    const int n_edges = *n_edges_dev;
    if (n_edges > max_edges) {
        if (lane == 0) { *found_out = -1; *err_out = 0.0; }
        for (int k = lane; k < cap; k += 64) { corr[2 * k] = -1; corr[2 * k + 1] = -1; }
        return;
    }
    int found;
    double err;
    rep_greedy_walk(keys, vals, n_edges, nd, vis_x, vis_y, kMaxPoints / 32, kMaxPoints / 32, corr, cap, found, err);
    if (lane == 0) { *found_out = found; *err_out = err; }
    for (int k = found + lane; k < cap; k += 64) { corr[2 * k] = -1; corr[2 * k + 1] = -1; }
}

__global__ void homography_kernel(const double *pts, int n, const double *h, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    homography_point(h, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], &out[4 * i], &out[4 * i + 1], &out[4 * i + 2]);
    out[4 * i + 3] = pts[4 * i + 3];
}

// Stable LSD radix sort of the candidate list, descending by overlap => equal overlaps stay in flat-index order
// (rep_sort_pairs, repeat_core.h), one workgroup of 16 waves.  The result always ends in (k1, v1).
// (Round 2 called hipcub::DeviceRadixSort here; the library now has no third-party device code.)
__global__ __launch_bounds__(kSortWaves * 64) void rep_sort_kernel(unsigned long long *k0, unsigned *v0, unsigned long long *k1,
                                                                  unsigned *v1, const int *n_dev, int max_edges) {
    __shared__ int hist[16][kSortWaves];
    __shared__ int uniform_digit;
    const int n = *n_dev;
    if (n <= 0 || n > max_edges) return;                          // nothing to sort / overflow (reported by rep_greedy_kernel)
    rep_sort_pairs(k0, v0, k1, v1, n, hist, &uniform_digit);
}

struct RepWs {
    int *cnt_s, *cnt_m, *poss, *off_s, *off_m, *totals;
    unsigned long long *key_s, *key_m, *key_out;      // candidate lists (both filled in one pass), sorted keys
    unsigned *val_s, *val_m, *val_out;
    size_t total;
};

RepWs rep_layout(char *base, int ns, int max_edges) {
    RepWs w{};
    WorkspaceCursor c{base, 0};
    const size_t rows = (size_t)ns * 4, e = (size_t)max_edges;
    w.cnt_s = c.take<int>(rows); w.cnt_m = c.take<int>(rows); w.poss = c.take<int>(rows);
    w.off_s = c.take<int>(rows); w.off_m = c.take<int>(rows); w.totals = c.take<int>(16);
    w.key_s = c.take<unsigned long long>(e * 8); w.key_m = c.take<unsigned long long>(e * 8);
    w.key_out = c.take<unsigned long long>(e * 8);
    w.val_s = c.take<unsigned>(e * 4); w.val_m = c.take<unsigned>(e * 4);
    w.val_out = c.take<unsigned>(e * 4);
    w.total = c.used;
    return w;
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_repeatability_workspace_bytes(int ns, int nd, int max_edges) {
    if (ns <= 0 || nd <= 0 || max_edges <= 0) return 0;
    return rep_layout(nullptr, ns, max_edges).total;
}

extern "C" int balf_repeatability(const double *src_dev, int ns, const double *dst_dev, int nd, double overlap_err,
                                  double eps, double dist_match_thresh, double radius_size, int max_edges,
                                  int32_t *counts_dev, double *errors_dev, int32_t *corr_s_dev, int32_t *corr_m_dev,
                                  void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!src_dev || !dst_dev || !counts_dev || !errors_dev || !corr_s_dev || !corr_m_dev || !workspace_dev) return BALF_ERR_ARG;
    if (ns <= 0 || nd <= 0 || max_edges <= 0 || ns > kMaxPoints || nd > kMaxPoints) return BALF_ERR_ARG;
    if ((long long)ns * nd > 0x7fffffffLL) return BALF_ERR_SHAPE;
    if (workspace_bytes < balf_repeatability_workspace_bytes(ns, nd, max_edges)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RepWs w = rep_layout(static_cast<char *>(workspace_dev), ns, max_edges);
    const RepParams p{1.0 - overlap_err, eps, dist_match_thresh, radius_size, 4.0 * radius_size};
    rep_count_kernel<<<ns, 256, 0, st>>>(src_dev, ns, dst_dev, nd, p, w.cnt_s, w.cnt_m, w.poss);
    BALF_LAUNCH_CHECK();
    rep_scan_kernel<<<1, 1024, 0, st>>>(w.cnt_s, w.cnt_m, w.poss, ns, w.off_s, w.off_m, w.totals, counts_dev + 2);
    BALF_LAUNCH_CHECK();
    // the list lengths stay on the device (round 5 read them back behind a hipStreamSynchronize): the fill pass cuts a list
    // at max_edges, the sort and assignment kernels read the length themselves
    rep_fill_kernel<<<ns, 64, 0, st>>>(src_dev, ns, dst_dev, nd, p, w.off_s, w.off_m, max_edges, w.key_s, w.val_s, w.key_m, w.val_m);
    BALF_LAUNCH_CHECK();
    const int cap = ns < nd ? ns : nd;
    for (int which = 0; which < 2; ++which) {
        // (sorts between the candidate list and the output buffers; the list is not needed again)
        rep_sort_kernel<<<1, kSortWaves * 64, 0, st>>>(which ? w.key_m : w.key_s, which ? w.val_m : w.val_s, w.key_out, w.val_out,
                                                      w.totals + which, max_edges);
        BALF_LAUNCH_CHECK();
        rep_greedy_kernel<<<1, 64, 0, st>>>(w.key_out, w.val_out, w.totals + which, max_edges, nd, counts_dev + which,
                                            errors_dev + which, which ? corr_m_dev : corr_s_dev, cap);
        BALF_LAUNCH_CHECK();
    }
    return BALF_OK;
}

extern "C" int balf_apply_homography(const double *points_dev, int n, const double *h_dev, double *out_dev, void *stream) {
    if (!points_dev || !h_dev || !out_dev || n <= 0) return BALF_ERR_ARG;
    homography_kernel<<<balf_ceil_div(n, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(points_dev, n, h_dev, out_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}


// create_common_region_masks (reference balf/benchmark_test/geometry_tools.py:7-26): the per-pixel body and the
// inverse maps are in common_mask.h (shared with the batched point filter of repeat_batch.hip).  cv2 is not installed in
// the build container: parity with it is UNPINNED (checked against the oracle's restatement of the same algorithm only).
namespace {

struct MaskArgs {
    double m[9];          // inverse map, row-major: output pixel -> input coordinates (homogeneous)
    int h_out, w_out;     // mask being produced
    int h_in, w_in;       // the all-ones image being warped
    int border;
    double *out;
};

__global__ __launch_bounds__(256) void common_mask_kernel(MaskArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.h_out * a.w_out) return;
    const int y = (int)(i / a.w_out), x = (int)(i - (long)y * a.w_out);
    a.out[i] = common_mask_pixel(a.m, y, x, a.h_out, a.w_out, a.h_in, a.w_in, a.border);
}

}  // namespace

extern "C" int balf_common_region_masks(const double *h_dst_2_src_host, int h_src, int w_src, int h_dst, int w_dst,
                                        int border, double *mask_src_dev, double *mask_dst_dev, void *stream) {
    if (!h_dst_2_src_host || !mask_src_dev || !mask_dst_dev) return BALF_ERR_ARG;
    if (h_src <= 0 || w_src <= 0 || h_dst <= 0 || w_dst <= 0 || border < 0) return BALF_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // mask_src = warp(ones_dst, M = h_dst_2_src): samples ones_dst at M^-1 (x, y, 1)
    // mask_dst = warp(ones_src, M = inv(h_dst_2_src) / its [2,2]): samples ones_src at M^-1 = a multiple of h_dst_2_src
    MaskArgs ms{}, md{};
    if (!common_mask_maps(h_dst_2_src_host, ms.m, md.m)) return BALF_ERR_ARG;
    ms.h_out = h_src; ms.w_out = w_src; ms.h_in = h_dst; ms.w_in = w_dst; ms.border = border; ms.out = mask_src_dev;
    md.h_out = h_dst; md.w_out = w_dst; md.h_in = h_src; md.w_in = w_src; md.border = border; md.out = mask_dst_dev;
    common_mask_kernel<<<balf_ceil_div((long)h_src * w_src, 256), 256, 0, st>>>(ms);
    BALF_LAUNCH_CHECK();
    common_mask_kernel<<<balf_ceil_div((long)h_dst * w_dst, 256), 256, 0, st>>>(md);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
