// Batched HSequences evaluation on gfx950: the per-pair body of check_val_hsequences_repeatability
// (balf/utils/train_utils.py:350-379) after detection, for P independent image pairs in one stream-ordered sequence of
// launches.  Nothing synchronises and nothing is read back; every per-pair length is read on the device.
//
//   balf_common_points_batch   check_common_points against both common-region masks (evaluated at the point only, through
//                              common_mask.h) + apply_homography_to_points of the kept destination rows (homography.h)
//     common_points_kernel     one workgroup per pair: both inverse maps, then an ordered compaction of each side
//                              (common_points.h, shared with balf_common_points_index_batch of match_eval.hip)
//   balf_repeatability_batch   compute_repeatability per pair, bit-identical to balf_repeatability (repeat_core.h)
//     rpb_count_kernel         one wave per (source row, pair): candidate counts and the "possible match" flag
//     rpb_row_scan_kernel      one workgroup per pair: exclusive scan of its row counts, the pair's totals
//     rpb_pair_scan_kernel     one workgroup: exclusive scan of the pair totals = each pair's slice of the candidate buffers
//     rpb_fill_kernel          one wave per (source row, pair): ordered compaction of the candidates into the pair's slice
//     rpb_sort_kernel          one workgroup per (pair, scale): the stable radix sort of the slice
//     rpb_greedy_kernel        one wave per (pair, scale): the greedy assignment walk
//     rpb_finalize_kernel      one thread per pair: the result fields with the reference's formulas
// The ordered compaction, the scans and the count clamp are the shared ones of block_ops.h.
#include "block_ops.h"
#include "common.h"
#include "common_points.h"
#include "repeat_core.h"

namespace balf {
namespace {

constexpr int kRowsPerBlock = 4;            // count / fill: one wave per source row

// One workgroup of 256 per pair: common_points_pair (common_points.h) without the row indices.
__global__ __launch_bounds__(256) void common_points_kernel(const double *src, const int *ns, int ns_max, const double *dst,
                                                            const int *nd, int nd_max, const double *h_all, const int *shapes,
                                                            double *src_out, double *dst_out, int *kept, int *valid) {
    __shared__ int wcnt[4];
    common_points_pair<false>(src, ns, ns_max, dst, nd, nd_max, h_all, shapes, src_out, dst_out, kept, valid, nullptr, nullptr,
                              wcnt);
}

struct BatchIn {
    const double *src, *dst;
    const int *ns, *nd;
    int ns_max, nd_max, src_stride, dst_stride, count_stride;
    __device__ int n_src(int p) const { return clamp_count(ns, (long)p * count_stride, ns_max); }
    __device__ int n_dst(int p) const { return clamp_count(nd, (long)p * count_stride, nd_max); }
};

__global__ __launch_bounds__(64 * kRowsPerBlock) void rpb_count_kernel(BatchIn in, RepParams rp, int *cnt_s, int *cnt_m, int *poss) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    const int ns = in.n_src(p), nd = in.n_dst(p);
    if (i >= ns) return;                                          // (a whole wave)
    const double *s = in.src + ((long)p * in.ns_max + i) * in.src_stride;
    const double *d = in.dst + (long)p * in.nd_max * in.dst_stride;
    const double sx = s[0], sy = s[1], sr = s[2];
    int cs = 0, cm = 0, ps = 0;
    for (int j = lane; j < nd; j += 64) {
        double so, mo; bool po;
        const double *t = d + (long)j * in.dst_stride;
        pair_overlaps(sx, sy, sr, t[0], t[1], t[2], rp, so, mo, po);
        cs += so >= rp.thr; cm += mo >= rp.thr; ps |= po;
    }
    cs = wave_sum(cs); cm = wave_sum(cm); ps = wave_sum(ps);
    if (lane == 0) {
        const long k = (long)p * in.ns_max + i;
        cnt_s[k] = cs; cnt_m[k] = cm; poss[k] = ps > 0;
    }
}

// one workgroup per pair: off[p, i] = sum_{k<i} cnt[p, k]; tot[p] = {sum cnt_s, sum cnt_m, sum poss}
__global__ __launch_bounds__(1024) void rpb_row_scan_kernel(BatchIn in, const int *cnt_s, const int *cnt_m, const int *poss,
                                                            int *off_s, int *off_m, int *tot) {
    __shared__ int wsum[3][16];
    __shared__ int base[3];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int ns = in.n_src(p);
    const int nd = in.n_dst(p);
    const int n = nd > 0 ? ns : 0;                                // no destination rows: every count is 0 (not computed)
    const long row0 = (long)p * in.ns_max;
    if (tid < 3) base[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const int v[3] = {i < n ? cnt_s[row0 + i] : 0, i < n ? cnt_m[row0 + i] : 0, i < n ? poss[row0 + i] : 0};
        int excl[3];
        block_scan_chunk<int, 3, 1024>(v, excl, wsum, base);
        if (i < n) { off_s[row0 + i] = excl[0]; off_m[row0 + i] = excl[1]; }
    }
    if (tid == 0) { tot[3 * p] = base[0]; tot[3 * p + 1] = base[1]; tot[3 * p + 2] = base[2]; }
}

// one workgroup: slice[p] = {sum_{q<p} tot[q][0], sum_{q<p} tot[q][1]} (64-bit: the sum over pairs may pass 2^31)
__global__ __launch_bounds__(1024) void rpb_pair_scan_kernel(const int *tot, int P, long long *slice) {
    __shared__ long long wsum[2][16];
    __shared__ long long base[2];
    const int tid = threadIdx.x;
    if (tid < 2) base[tid] = 0;
    __syncthreads();
    for (int p0 = 0; p0 < P; p0 += 1024) {
        const int p = p0 + tid;
        const long long v[2] = {p < P ? (long long)tot[3 * p] : 0, p < P ? (long long)tot[3 * p + 1] : 0};
        long long excl[2];
        block_scan_chunk<long long, 2, 1024>(v, excl, wsum, base);
        if (p < P) { slice[2 * p] = excl[0]; slice[2 * p + 1] = excl[1]; }
    }
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void rpb_fill_kernel(BatchIn in, RepParams rp, const int *off_s, const int *off_m,
                                                                      const long long *slice, int max_edges,
                                                                      unsigned long long *key_s, unsigned *val_s,
                                                                      unsigned long long *key_m, unsigned *val_m) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    const int ns = in.n_src(p), nd = in.n_dst(p);
    if (i >= ns) return;                                          // (a whole wave)
    const double *s = in.src + ((long)p * in.ns_max + i) * in.src_stride;
    const double *d = in.dst + (long)p * in.nd_max * in.dst_stride;
    const double sx = s[0], sy = s[1], sr = s[2];
    long long ws = slice[2 * p] + off_s[(long)p * in.ns_max + i], wm = slice[2 * p + 1] + off_m[(long)p * in.ns_max + i];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j0 = 0; j0 < nd; j0 += 64) {
        const int j = j0 + lane;
        double so = 0.0, mo = 0.0; bool po;
        if (j < nd) { const double *t = d + (long)j * in.dst_stride; pair_overlaps(sx, sy, sr, t[0], t[1], t[2], rp, so, mo, po); }
        const bool ks = j < nd && so >= rp.thr, km = j < nd && mo >= rp.thr;
        const unsigned long long bs = __ballot(ks), bm = __ballot(km);
        // a slice that runs past max_edges is cut here and reported by rpb_greedy_kernel (found -1); the entries cut away
        // belong to no other pair's slice (slices are disjoint and in pair order)
        if (ks) { const long long o = ws + __popcll(bs & below); if (o < max_edges) { key_s[o] = __double_as_longlong(so); val_s[o] = (unsigned)(i * nd + j); } }
        if (km) { const long long o = wm + __popcll(bm & below); if (o < max_edges) { key_m[o] = __double_as_longlong(mo); val_m[o] = (unsigned)(i * nd + j); } }
        ws += __popcll(bs); wm += __popcll(bm);
    }
}

__device__ __forceinline__ bool slice_fits(const int *tot, const long long *slice, int p, int which, int max_edges) {
    return slice[2 * p + which] + tot[3 * p + which] <= (long long)max_edges;
}

// grid (P, 2): the candidate slice of (pair, scale) from (k0, v0) sorted into the same slice of (k1, v1)
__global__ __launch_bounds__(kSortWaves * 64) void rpb_sort_kernel(unsigned long long *k0_s, unsigned *v0_s, unsigned long long *k0_m,
                                                                  unsigned *v0_m, unsigned long long *k1_s, unsigned *v1_s,
                                                                  unsigned long long *k1_m, unsigned *v1_m, const int *tot,
                                                                  const long long *slice, int max_edges) {
    __shared__ int hist[16][kSortWaves];
    __shared__ int uniform_digit;
    const int p = blockIdx.x, which = blockIdx.y;
    const int n = tot[3 * p + which];
    if (n <= 0 || !slice_fits(tot, slice, p, which, max_edges)) return;      // nothing to sort / overflow (rpb_greedy_kernel)
    const long long o = slice[2 * p + which];
    rep_sort_pairs((which ? k0_m : k0_s) + o, (which ? v0_m : v0_s) + o, (which ? k1_m : k1_s) + o, (which ? v1_m : v1_s) + o,
                   n, hist, &uniform_digit);
}

// grid (P, 2), one wave each: found[p][which] (-1: the slice did not fit), err[p][which]
__global__ __launch_bounds__(64) void rpb_greedy_kernel(BatchIn in, const unsigned long long *k_s, const unsigned *v_s,
                                                        const unsigned long long *k_m, const unsigned *v_m, const int *tot,
                                                        const long long *slice, int max_edges, int *found_out, double *err_out) {
    __shared__ unsigned vis_x[kMaxPoints / 32], vis_y[kMaxPoints / 32];
    const int p = blockIdx.x, which = blockIdx.y, lane = threadIdx.x;
    const int n = tot[3 * p + which];
    if (!slice_fits(tot, slice, p, which, max_edges)) {
        if (lane == 0) { found_out[2 * p + which] = -1; err_out[2 * p + which] = 0.0; }
        return;
    }
    const int ns = in.n_src(p), nd = in.n_dst(p);
    const long long o = slice[2 * p + which];
    int found = 0;
    double err = 0.0;
    if (n > 0)
        rep_greedy_walk((which ? k_m : k_s) + o, (which ? v_m : v_s) + o, n, nd, vis_x, vis_y, (nd + 31) / 32, (ns + 31) / 32,
                        nullptr, 0, found, err);
    if (lane == 0) { found_out[2 * p + which] = found; err_out[2 * p + which] = err; }
}

// repeatability_tools.py:379-490 as balf_amd/benchmark_test/repeatability_tools.py:61-64 restates them:
//   rep = found / float(total) * 100 (NaN for total 0), err = 0 if found == 0 else err_sum / (found + np.finfo(float).eps)
__global__ __launch_bounds__(256) void rpb_finalize_kernel(BatchIn in, int P, const int *tot, const int *found, const double *err,
                                                           double *rep_out, int *counts_out) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int ns = in.n_src(p), nd = in.n_dst(p);
    const int total = ns < nd ? ns : nd;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int which = 0; which < 2; ++which) {
        const int f = found[2 * p + which];
        const double e = err[2 * p + which];
        rep_out[4 * p + which] = f < 0 ? nan : (double)f / (double)total * 100.0;
        rep_out[4 * p + 2 + which] = f < 0 ? nan : (f == 0 ? 0.0 : e / ((double)f + kEpsF64));
        counts_out[6 * p + which] = f;
        counts_out[6 * p + 4 + which] = tot[3 * p + which];
    }
    counts_out[6 * p + 2] = tot[3 * p + 2];
    counts_out[6 * p + 3] = total;
}

struct RpbWs {
    int *cnt_s, *cnt_m, *poss, *off_s, *off_m, *tot, *found;
    long long *slice;
    double *err;
    unsigned long long *key_s, *key_m, *out_key_s, *out_key_m;
    unsigned *val_s, *val_m, *out_val_s, *out_val_m;
    size_t total;
};

RpbWs rpb_layout(char *base, int P, int ns_max, int max_edges) {
    RpbWs w{};
    WorkspaceCursor c{base, 0};
    const size_t rows = (size_t)P * ns_max, e = (size_t)max_edges;
    w.cnt_s = c.take<int>(rows * 4); w.cnt_m = c.take<int>(rows * 4); w.poss = c.take<int>(rows * 4);
    w.off_s = c.take<int>(rows * 4); w.off_m = c.take<int>(rows * 4);
    w.tot = c.take<int>((size_t)P * 12); w.found = c.take<int>((size_t)P * 8);
    w.slice = c.take<long long>((size_t)P * 16); w.err = c.take<double>((size_t)P * 16);
    w.key_s = c.take<unsigned long long>(e * 8); w.key_m = c.take<unsigned long long>(e * 8);
    w.out_key_s = c.take<unsigned long long>(e * 8); w.out_key_m = c.take<unsigned long long>(e * 8);
    w.val_s = c.take<unsigned>(e * 4); w.val_m = c.take<unsigned>(e * 4);
    w.out_val_s = c.take<unsigned>(e * 4); w.out_val_m = c.take<unsigned>(e * 4);
    w.total = c.used;
    return w;
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" int balf_common_points_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, const double *dst_dev,
                                        const int32_t *nd_dev, int nd_max, int P, const double *h_dst_2_src_dev,
                                        const int32_t *shapes_dev, double *src_out_dev, double *dst_out_dev,
                                        int32_t *kept_dev, int32_t *valid_dev, void *stream) {
    if (!src_dev || !ns_dev || !dst_dev || !nd_dev || !h_dst_2_src_dev || !shapes_dev || !src_out_dev || !dst_out_dev ||
        !kept_dev || !valid_dev)
        return BALF_ERR_ARG;
    const int rc = check_sizes(P, ns_max, nd_max);
    if (rc != BALF_OK) return rc;
    common_points_kernel<<<P, 256, 0, static_cast<hipStream_t>(stream)>>>(src_dev, ns_dev, ns_max, dst_dev, nd_dev, nd_max,
                                                                          h_dst_2_src_dev, shapes_dev, src_out_dev, dst_out_dev,
                                                                          kept_dev, valid_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" size_t balf_repeatability_batch_workspace_bytes(int P, int ns_max, int nd_max, int max_edges) {
    if (check_sizes(P, ns_max, nd_max) != BALF_OK || max_edges <= 0) return 0;
    return rpb_layout(nullptr, P, ns_max, max_edges).total;
}

extern "C" int balf_repeatability_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, int src_stride,
                                        const double *dst_dev, const int32_t *nd_dev, int nd_max, int dst_stride,
                                        int count_stride, int P, double overlap_err, double eps, double dist_match_thresh,
                                        double radius_size, int max_edges, double *rep_dev, int32_t *counts_dev,
                                        void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!src_dev || !ns_dev || !dst_dev || !nd_dev || !rep_dev || !counts_dev || !workspace_dev) return BALF_ERR_ARG;
    if (src_stride < 3 || dst_stride < 3 || count_stride < 1 || max_edges <= 0) return BALF_ERR_ARG;
    const int rc = check_sizes(P, ns_max, nd_max);
    if (rc != BALF_OK) return rc;
    if (workspace_bytes < balf_repeatability_batch_workspace_bytes(P, ns_max, nd_max, max_edges)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RpbWs w = rpb_layout(static_cast<char *>(workspace_dev), P, ns_max, max_edges);
    const RepParams rp{1.0 - overlap_err, eps, dist_match_thresh, radius_size, 4.0 * radius_size};
    const BatchIn in{src_dev, dst_dev, ns_dev, nd_dev, ns_max, nd_max, src_stride, dst_stride, count_stride};
    const dim3 rows_grid(balf_ceil_div(ns_max, kRowsPerBlock), P);
    if (ns_max > 0 && nd_max > 0) {
        rpb_count_kernel<<<rows_grid, 64 * kRowsPerBlock, 0, st>>>(in, rp, w.cnt_s, w.cnt_m, w.poss);
        BALF_LAUNCH_CHECK();
    }
    rpb_row_scan_kernel<<<P, 1024, 0, st>>>(in, w.cnt_s, w.cnt_m, w.poss, w.off_s, w.off_m, w.tot);
    BALF_LAUNCH_CHECK();
    rpb_pair_scan_kernel<<<1, 1024, 0, st>>>(w.tot, P, w.slice);
    BALF_LAUNCH_CHECK();
    if (ns_max > 0 && nd_max > 0) {
        rpb_fill_kernel<<<rows_grid, 64 * kRowsPerBlock, 0, st>>>(in, rp, w.off_s, w.off_m, w.slice, max_edges, w.key_s, w.val_s,
                                                                  w.key_m, w.val_m);
        BALF_LAUNCH_CHECK();
    }
    rpb_sort_kernel<<<dim3(P, 2), kSortWaves * 64, 0, st>>>(w.key_s, w.val_s, w.key_m, w.val_m, w.out_key_s, w.out_val_s,
                                                           w.out_key_m, w.out_val_m, w.tot, w.slice, max_edges);
    BALF_LAUNCH_CHECK();
    rpb_greedy_kernel<<<dim3(P, 2), 64, 0, st>>>(in, w.out_key_s, w.out_val_s, w.out_key_m, w.out_val_m, w.tot, w.slice,
                                                max_edges, w.found, w.err);
    BALF_LAUNCH_CHECK();
    rpb_finalize_kernel<<<balf_ceil_div(P, 256), 256, 0, st>>>(in, P, w.tot, w.found, w.err, rep_dev, counts_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
