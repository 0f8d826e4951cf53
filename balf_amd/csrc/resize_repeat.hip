// The resize protocol of the HSequences evaluation on gfx950 (balf/configs/config_hpatches.py: parse_resize_eval_config):
//   balf_resize_crop_u8                  ratio_preserving_resize (balf/datasets/dataset_utils.py:15-27) of B uint8 images of
//                                        different sizes into one [B, th, tw, C] batch, one launch
//   balf_resize_repeatability_batch      compute_resize_repeatability (balf/benchmark_test/repeatability_tools.py:516-614) for
//                                        P pairs, stream-ordered, nothing read back, every per-pair length read on the device
//     rr_select_kernel    one workgroup per (pair, side): the side's rows warped (homography.h's numerator / denominator
//                         expressions) and tested against the other image's shape; the keep_k_points rows of highest prob by an
//                         MSB-first radix select on the monotone 64-bit key of the float64 prob (ties at the cut: the lower
//                         original index, a second select); ordered compaction of the kept (row, col) into the workspace
//                         (block_sum, radix_select and compact_slot of block_ops.h)
//     rr_min_kernel       grid (64-row tiles, 2 directions, P), 4 waves per workgroup: every wave takes the same 64 kept rows
//                         of one side (one per lane) against a quarter of the other side's kept rows, staged in LDS in tiles
//                         (every lane reads the same address: a broadcast); min of dx*dx + dy*dy, one sqrt per row.  Run with
//                         the roles swapped for the column minima: no float atomics, no order dependence (min is exact)
//     rr_finalize_kernel  one workgroup per pair: counts and sums of the minima within the threshold in ONE fixed order (thread
//                         t sums rows t, t + 256, ...; then a fixed tree), so a pair's result does not depend on P or on its
//                         place in the batch; the result fields with the reference's formulas
// fp contraction is OFF wherever a float64 expression is compared against the reference (warps, distances, results).
#include "block_ops.h"
#include "common.h"
#include "homography.h"

namespace balf {
namespace {

constexpr int kSelThreads = 1024;
constexpr int kMaxRows = 65536;             // rows per side and pair
constexpr int kMinRows = 64;                // rows per workgroup of rr_min_kernel (one per lane)
constexpr int kMinWaves = 4;                // ... each wave a quarter of the columns
constexpr int kMinTile = 1024;              // columns staged in LDS at a time (16 KB)
constexpr int kFinThreads = 256;

struct RrSide {
    const double *rows;                     // [P, n_max, stride]
    const int *count;                       // [P * count_stride]
    int n_max, stride;
    unsigned long long *keys;               // [P, n_max] workspace: 0 = outside the common region
};

struct RrArgs {
    RrSide side[2];                         // 0 source, 1 destination
    int count_stride, order_xy, K, kcap;
    const double *h, *h_inv;                // [P, 9]
    const int *shapes;                      // [P, 4]
    double *kept;                           // [P, 2, kcap, 2] (row, col)
    int *kept_n;                            // [P, 2]
};

// order-preserving map of a float64 onto unsigned: a < b  <=>  key(a) < key(b); never 0 (0 marks a dropped row).  -0.0 takes
// the key of +0.0: the two compare equal, so between them the lower row index decides, as in NumPy's stable argsort.  NaN has
// no place in the order: probs are finite by contract.
__device__ __forceinline__ unsigned long long prob_key(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    if ((b << 1) == 0ull) b = 0ull;                              // -0.0 -> +0.0
    const unsigned long long k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return k ? k : 1ull;
}

// One row of one side: (row, col, prob) as read, and what goes on when it is inside the common region.
//   source (sd 0): warped with H on (col, row); kept when the WARPED point is inside shape_dst; the warped (row, col) goes on
//   destination (sd 1): warped with inv(H); kept when the warped point is inside shape_src; the UNWARPED (row, col) goes on
__device__ __forceinline__ bool side_point(const double *r, int order_xy, int sd, const double *m, int h_lim, int w_lim,
                                           double *o_row, double *o_col, double *prob) {
#pragma clang fp contract(off)
    const double row = order_xy ? r[1] : r[0], col = order_xy ? r[0] : r[1];
    *prob = order_xy ? r[3] : r[2];
    const double den = m[6] * col + m[7] * row + m[8];
    const double nx = m[0] * col + m[1] * row + m[2], ny = m[3] * col + m[4] * row + m[5];
    const double wc = nx / den, wr = ny / den;
    *o_row = sd ? row : wr;
    *o_col = sd ? col : wc;
    return wr >= 0.0 && wr < (double)h_lim && wc >= 0.0 && wc < (double)w_lim;
}

// grid (P, 2): blockIdx.y = side (0 source, 1 destination)
__global__ __launch_bounds__(kSelThreads) void rr_select_kernel(RrArgs a) {
    __shared__ unsigned s_hist[256];
    __shared__ int s_tmp[4];
    __shared__ int s_red[kSelThreads / 64];
    const int p = blockIdx.x, sd = blockIdx.y, tid = threadIdx.x;
    const RrSide &s = a.side[sd];
    const int n = clamp_count(s.count, (long)p * a.count_stride, s.n_max);
    const double *rows = s.rows + (long)p * s.n_max * s.stride;
    unsigned long long *keys = s.keys + (long)p * s.n_max;
    const double *m = (sd ? a.h_inv : a.h) + 9 * (long)p;
    // the image the warped point must fall into: the destination's for source rows, the source's for destination rows
    const int h_lim = a.shapes[4 * p + (sd ? 0 : 2)], w_lim = a.shapes[4 * p + (sd ? 1 : 3)];

    // 1. the common region: a key per row, 0 outside
    int mine = 0;
    for (int i = tid; i < n; i += kSelThreads) {
        double orow, ocol, prob;
        const bool in = side_point(rows + (long)i * s.stride, a.order_xy, sd, m, h_lim, w_lim, &orow, &ocol, &prob);
        keys[i] = in ? prob_key(prob) : 0ull;
        mine += in;
    }
    const int n_in = block_sum<kSelThreads>(mine, s_red);        // (its barriers also order the stores above before step 2)

    // 2. select_k_best: key > thr, or key == thr with index <= idx_cut (higher prob first, then the lower original index)
    unsigned long long thr = 1ull;
    int idx_cut = 0x7fffffff;
    if (n_in > a.K) {
        int n_eq, need_eq;
        thr = radix_select<64, true, kSelThreads>(
            a.K,
            [&](auto count) {
                for (int i = tid; i < n; i += kSelThreads) {
                    const unsigned long long k = keys[i];
                    if (k != 0ull) count(k);
                }
            },
            s_hist, s_tmp, &n_eq, &need_eq);
        if (n_eq > need_eq) {
            int d0, d1;
            const unsigned long long t = thr;
            idx_cut = (int)radix_select<32, false, kSelThreads>(
                need_eq,
                [&](auto count) {
                    for (int i = tid; i < n; i += kSelThreads)
                        if (keys[i] == t) count((unsigned)i);
                },
                s_hist, s_tmp, &d0, &d1);
        }
    }

    // 3. ordered compaction of the kept rows (original order: the finalize sums depend on nothing else)
    double *out = a.kept + ((long)p * 2 + sd) * a.kcap * 2;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += kSelThreads) {
        const int i = i0 + tid;
        bool keep = false;
        if (i < n) {
            const unsigned long long k = keys[i];
            keep = k != 0ull && (k > thr || (k == thr && i <= idx_cut));
        }
        const int q = compact_slot<kSelThreads>(keep, s_red, base);
        if (keep && q < a.kcap) {                                // (always: at most min(K, n_max) rows are kept)
            double orow, ocol, prob;
            side_point(rows + (long)i * s.stride, a.order_xy, sd, m, h_lim, w_lim, &orow, &ocol, &prob);
            out[2 * q] = orow;
            out[2 * q + 1] = ocol;
        }
    }
    if (tid == 0) a.kept_n[2 * p + sd] = base < a.kcap ? base : a.kcap;
}

// grid (ceil(kcap / 64), 2, P): blockIdx.y = 0: rows = kept source rows, columns = kept destination rows (min1); 1: swapped
__global__ __launch_bounds__(kMinRows * kMinWaves) void rr_min_kernel(const double *kept, const int *kept_n, int kcap,
                                                                      double *mins /*[P, 2, kcap]*/) {
#pragma clang fp contract(off)
    __shared__ double2 s_col[kMinTile];
    __shared__ double s_min[kMinWaves][kMinRows];
    const int p = blockIdx.z, dir = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_row = kept_n[2 * p + dir], n_col = kept_n[2 * p + (dir ^ 1)];
    const int r0 = blockIdx.x * kMinRows;
    if (r0 >= n_row || n_col == 0) return;                       // (the whole workgroup; no columns: the minima are not used)
    const double2 *rows = reinterpret_cast<const double2 *>(kept) + ((long)p * 2 + dir) * kcap;
    const double2 *cols = reinterpret_cast<const double2 *>(kept) + ((long)p * 2 + (dir ^ 1)) * kcap;
    const int r = r0 + lane;
    const double2 me = r < n_row ? rows[r] : make_double2(0.0, 0.0);
    double best = __longlong_as_double(0x7ff0000000000000LL);    // +inf
    for (int c0 = 0; c0 < n_col; c0 += kMinTile) {
        const int nt = n_col - c0 < kMinTile ? n_col - c0 : kMinTile;
        __syncthreads();                                         // the previous tile has been read
        for (int j = threadIdx.x; j < nt; j += kMinRows * kMinWaves) s_col[j] = cols[c0 + j];
        __syncthreads();
        for (int j = wave; j < nt; j += kMinWaves) {
            const double2 c = s_col[j];
            const double dy = me.x - c.x, dx = me.y - c.y;
            const double d2 = dy * dy + dx * dx;
            best = d2 < best ? d2 : best;
        }
    }
    s_min[wave][lane] = best;
    __syncthreads();
    if (wave == 0 && r < n_row) {
#pragma unroll
        for (int w = 1; w < kMinWaves; ++w) best = s_min[w][lane] < best ? s_min[w][lane] : best;
        mins[((long)p * 2 + dir) * kcap + r] = sqrt(best);
    }
}

// grid P.  rep_out [P, 2] = (repeatability, localization_err); counts_out [P, 4] = (N1, N2, count1, count2)
__global__ __launch_bounds__(kFinThreads) void rr_finalize_kernel(const double *mins, const int *kept_n, int kcap, double thresh,
                                                                  double *rep_out, int *counts_out) {
#pragma clang fp contract(off)
    __shared__ double s_sum[kFinThreads];
    __shared__ int s_cnt[kFinThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n1 = kept_n[2 * p], n2 = kept_n[2 * p + 1];
    int count[2];
    double sum[2];
    for (int dir = 0; dir < 2; ++dir) {
        const int n = (dir ? n1 : n2) != 0 ? (dir ? n2 : n1) : 0;            // `if N2 != 0` / `if N1 != 0`
        const double *m = mins + ((long)p * 2 + dir) * kcap;
        double s = 0.0;
        int c = 0;
        for (int i = tid; i < n; i += kFinThreads) {
            const double v = m[i];
            if (v <= thresh) { s = s + v; ++c; }
        }
        __syncthreads();                                         // the previous direction has been read
        s_sum[tid] = s;
        s_cnt[tid] = c;
        __syncthreads();
        for (int o = kFinThreads / 2; o > 0; o >>= 1) {
            if (tid < o) { s_sum[tid] = s_sum[tid] + s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
            __syncthreads();
        }
        sum[dir] = s_sum[0];
        count[dir] = s_cnt[0];
    }
    if (tid == 0) {
        const int c = count[0] + count[1];
        double rep = 0.0, err = -1.0;
        if (c > 0) {                                             // (then N1 + N2 > 0)
            rep = (double)c / (double)(n1 + n2) * 100.0;
            err = sum[0] / (double)c + sum[1] / (double)c;
        }
        rep_out[2 * p] = rep;
        rep_out[2 * p + 1] = err;
        counts_out[4 * p] = n1;
        counts_out[4 * p + 1] = n2;
        counts_out[4 * p + 2] = count[0];
        counts_out[4 * p + 3] = count[1];
    }
}

struct RrWs {
    unsigned long long *keys_s, *keys_d;
    double *kept, *mins;
    int *kept_n;
    size_t total;
};

int kept_cap(int ns_max, int nd_max, int K) {
    const int n = ns_max > nd_max ? ns_max : nd_max;
    const int c = K < n ? K : n;
    return c < 1 ? 1 : c;
}

RrWs rr_layout(char *base, int P, int ns_max, int nd_max, int K) {
    RrWs w{};
    WorkspaceCursor c{base, 0};
    const size_t kcap = (size_t)kept_cap(ns_max, nd_max, K);
    w.keys_s = c.take<unsigned long long>((size_t)P * ns_max * 8);
    w.keys_d = c.take<unsigned long long>((size_t)P * nd_max * 8);
    w.kept = c.take<double>((size_t)P * 2 * kcap * 16);
    w.mins = c.take<double>((size_t)P * 2 * kcap * 8);
    w.kept_n = c.take<int>((size_t)P * 8);
    w.total = c.used;
    return w;
}

int check_sizes(int P, int ns_max, int nd_max, int K) {
    if (P <= 0 || P > kMaxPairs || ns_max < 0 || nd_max < 0 || ns_max > kMaxRows || nd_max > kMaxRows || K <= 0 ||
        K > BALF_MAX_TOPK)
        return BALF_ERR_ARG;
    return BALF_OK;
}

// ---- ratio_preserving_resize --------------------------------------------------------------------------------------------------
struct ResizeGeom {
    int new_h, new_w, top, left;
};

// new size (np.round: half to even) and the offsets of the centred crop / pad.  The reference hands
// (hp, wp, th - new_h - hp, tw - new_w - wp) to imgaug's CropAndPad, whose order is (top, RIGHT, bottom, LEFT): the top offset is
// hp = floor((th - new_h) / 2) and the left one tw - new_w - floor((tw - new_w) / 2).
__host__ __device__ __forceinline__ ResizeGeom resize_geom(int h, int w, int th, int tw) {
    const double sh = (double)th / (double)h, sw = (double)tw / (double)w;
    const double scale = sh > sw ? sh : sw;
    ResizeGeom g;
    g.new_h = (int)rint((double)h * scale);
    g.new_w = (int)rint((double)w * scale);
    const int dh = th - g.new_h, dw = tw - g.new_w;
    const int hp = dh >= 0 ? dh / 2 : -((-dh + 1) / 2), wp = dw >= 0 ? dw / 2 : -((-dw + 1) / 2);   // floor division
    g.top = hp;
    g.left = dw - wp;
    return g;
}

// the source tap and the two 11-bit weights of output coordinate d on one axis (OpenCV's INTER_LINEAR set-up, as documented)
__device__ __forceinline__ void linear_tap(int d, int n_src, int n_new, int *s0, int *s1, int *w0, int *w1) {
#pragma clang fp contract(off)
    const double ratio = (double)n_src / (double)n_new;
    float f = (float)(((double)d + 0.5) * ratio - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.0f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.0f; }
    *s0 = s;
    *s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    *w0 = (int)rintf((1.0f - f) * 2048.0f);
    *w1 = (int)rintf(f * 2048.0f);
}

// grid (ceil(tw / 64), ceil(th / 4), B), block (64, 4): one output pixel per thread, all channels
__global__ __launch_bounds__(256) void resize_crop_kernel(const unsigned char *packed, size_t packed_bytes, const long long *offsets,
                                                          const int *sizes, int C, int th, int tw, unsigned char *out) {
    const int b = blockIdx.z, x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= tw || y >= th) return;
    unsigned char *o = out + (((long)b * th + y) * tw + x) * C;
    const int h = sizes[2 * b], w = sizes[2 * b + 1];
    const long long off = offsets[b];
    bool ok = h > 0 && w > 0 && off >= 0 && (unsigned long long)off + (unsigned long long)h * w * C <= packed_bytes;
    int ry = 0, rx = 0;
    ResizeGeom g{};
    if (ok) {
        g = resize_geom(h, w, th, tw);
        ry = y - g.top;
        rx = x - g.left;
        ok = ry >= 0 && ry < g.new_h && rx >= 0 && rx < g.new_w;
    }
    if (!ok) {                                                   // zero pad (and an image that does not lie inside the buffer)
        for (int c = 0; c < C; ++c) o[c] = 0;
        return;
    }
    int x0, x1, a0, a1, y0, y1, b0, b1;
    linear_tap(rx, w, g.new_w, &x0, &x1, &a0, &a1);
    linear_tap(ry, h, g.new_h, &y0, &y1, &b0, &b1);
    const unsigned char *r0 = packed + off + (long)y0 * w * C, *r1 = packed + off + (long)y1 * w * C;
    for (int c = 0; c < C; ++c) {
        const int s0 = r0[x0 * C + c] * a0 + r0[x1 * C + c] * a1;
        const int s1 = r1[x0 * C + c] * a0 + r1[x1 * C + c] * a1;
        const int v = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;
        o[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_resize_repeatability_batch_workspace_bytes(int P, int ns_max, int nd_max, int keep_k_points) {
    if (check_sizes(P, ns_max, nd_max, keep_k_points) != BALF_OK) return 0;
    return rr_layout(nullptr, P, ns_max, nd_max, keep_k_points).total;
}

extern "C" int balf_resize_repeatability_batch(const double *src_dev, const int32_t *ns_dev, int ns_max, int src_stride,
                                               const double *dst_dev, const int32_t *nd_dev, int nd_max, int dst_stride,
                                               int count_stride, int order_xy, int P, const double *h_dev,
                                               const double *h_inv_dev, const int32_t *shapes_dev, int keep_k_points,
                                               double distance_thresh, double *rep_dev, int32_t *counts_dev,
                                               void *workspace_dev, size_t workspace_bytes, void *stream) {
    // (a side without rows, n_max == 0, may come with a null pointer: an empty tensor has none)
    if ((!src_dev && ns_max != 0) || !ns_dev || (!dst_dev && nd_max != 0) || !nd_dev || !h_dev || !h_inv_dev || !shapes_dev ||
        !rep_dev || !counts_dev || !workspace_dev)
        return BALF_ERR_ARG;
    const int min_stride = order_xy ? 4 : 3;
    if ((order_xy != 0 && order_xy != 1) || src_stride < min_stride || dst_stride < min_stride || count_stride < 1 ||
        !(distance_thresh >= 0.0))
        return BALF_ERR_ARG;
    const int rc = check_sizes(P, ns_max, nd_max, keep_k_points);
    if (rc != BALF_OK) return rc;
    if (workspace_bytes < balf_resize_repeatability_batch_workspace_bytes(P, ns_max, nd_max, keep_k_points))
        return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RrWs w = rr_layout(static_cast<char *>(workspace_dev), P, ns_max, nd_max, keep_k_points);
    RrArgs a{};
    a.side[0] = RrSide{src_dev, ns_dev, ns_max, src_stride, w.keys_s};
    a.side[1] = RrSide{dst_dev, nd_dev, nd_max, dst_stride, w.keys_d};
    a.count_stride = count_stride;
    a.order_xy = order_xy;
    a.K = keep_k_points;
    a.kcap = kept_cap(ns_max, nd_max, keep_k_points);
    a.h = h_dev;
    a.h_inv = h_inv_dev;
    a.shapes = shapes_dev;
    a.kept = w.kept;
    a.kept_n = w.kept_n;
    rr_select_kernel<<<dim3(P, 2), kSelThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    rr_min_kernel<<<dim3(balf_ceil_div(a.kcap, kMinRows), 2, P), kMinRows * kMinWaves, 0, st>>>(w.kept, w.kept_n, a.kcap, w.mins);
    BALF_LAUNCH_CHECK();
    rr_finalize_kernel<<<P, kFinThreads, 0, st>>>(w.mins, w.kept_n, a.kcap, distance_thresh, rep_dev, counts_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_resize_crop_u8(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                                   const int32_t *sizes_dev, int B, int channels, int target_h, int target_w,
                                   unsigned char *out_dev, void *stream) {
    if (!packed_dev || !offsets_dev || !sizes_dev || !out_dev) return BALF_ERR_ARG;
    if (B <= 0 || B > kMaxPairs /* B is grid z */ || (channels != 1 && channels != 3) || target_h <= 0 || target_w <= 0)
        return BALF_ERR_ARG;
    if (target_h > 16384 || target_w > 16384) return BALF_ERR_SHAPE;
    resize_crop_kernel<<<dim3(balf_ceil_div(target_w, 64), balf_ceil_div(target_h, 4), B), dim3(64, 4), 0,
                         static_cast<hipStream_t>(stream)>>>(packed_dev, packed_bytes, offsets_dev, sizes_dev, channels, target_h,
                                                             target_w, out_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
