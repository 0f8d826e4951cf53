// The synthetic-homography image pairs of the validation task on gfx950 (balf/datasets/COCO.py:42-205, GOPRO inherits it):
//   balf_synth_pairs    P pairs per call, stream-ordered, nothing read back, two launches
//     synth_image_kernel   grid (ceil(patch * ceil(patch / 4) / 256), 2 sides, P), 256 threads, FOUR consecutive output pixels
//                          of one row per thread: the three planes of an image patch are written as one 16-byte store per
//                          plane and thread (a wave writes 1 KiB of a row), the side's heat-map tile is zeroed the same way.
//                            side 0  the source window: byte / 255, planar
//                            side 1  cv2.warpPerspective(src, inv_h) with default flags (bilinear, constant-zero border) for
//                                    8-bit 3-channel data, evaluated at the destination window's pixels only.  The source
//                                    coordinate of an output pixel is warp_source_q5 (common_mask.h) under invert3(inv_h),
//                                    the one the common-region masks sample; weights are the exact integer products of the
//                                    5-bit fractions, (32 - fx)(32 - fy) * 32 ... (they sum to 32768, so OpenCV's correction
//                                    of the weight table never fires), a tap outside the source contributes 0, the pixel is
//                                    (sum + 16384) >> 15.  The largest 8-bit value of the workgroup goes to the workspace.
//                          The taps are read straight from global memory as bytes (2 x 2 locality, neighbouring lanes share
//                          cache lines); the footprint is not staged in LDS: the kernel is bound by the float32 stores, 32
//                          bytes written per 3 bytes read.  byte / 255 comes from a 256-entry LDS table every
//                          workgroup computes with the reference's expression, (float)((double)v / 255.0).
//     synth_labels_kernel  one workgroup of 1024 threads per pair, AFTER the image kernel (the heat maps are zero by then):
//                          select_k_best (dataset_utils.py:277-286) by radix_select (block_ops.h) on the monotone 32-bit key of
//                          prob, ties at the cut: the lower row index (a second select); the kept points truncated to integers;
//                          1.0 at the ones inside the source window (labels_to_heatmap, :288-292); warped with inv_h narrowed
//                          to float32 in float32 arithmetic, kept inside the FULL image, rounded half to even, 1.0 at the ones
//                          inside the destination window (apply_homography_to_source_labels_torch as it returns, :200-219).
//                          Every store is 1.0f: duplicates need no atomics and no order.  The workgroup maxima of the image
//                          kernel are reduced to dst_max (max is exact: no order dependence).
// This follows OpenCV's 8-bit INTER_LINEAR remap as documented; parity with cv2 itself is UNPINNED (checked against the
// tests' integer restatement of the same algorithm only), like the masks (common_mask.h) and the resize (resize_repeat.hip).
// fp contraction is OFF wherever a float expression is compared against the reference (the label warp; common_mask.h).
#include "block_ops.h"
#include "common.h"
#include "common_mask.h"

namespace balf {
namespace {

constexpr int kImgThreads = 256;
constexpr int kImgPx = 4;                   // output pixels per thread: one 16-byte store per plane
constexpr int kLblThreads = 1024;
constexpr int kMaxPatch = 16384;

struct SynthArgs {
    const unsigned char *packed;
    size_t packed_bytes;
    const long long *offsets;               // [P]
    const int *sizes;                       // [P, 2] (h, w)
    const double *inv_h;                    // [P, 9]
    const int *win_src, *win_dst;           // [P, 2] (top, left)
    const float *pts;                       // [pts_total, 3] (x, y, prob)
    const int *pts_off;                     // [P + 1]
    int pts_total, top_k, patch, nblk, vec;
    float *img_src, *img_dst;               // [P, 3, patch, patch]
    float *heat_src, *heat_dst;             // [P, 1, patch, patch]
    int *dst_max;                           // [P]
    int *blk_max;                           // [P, nblk] workspace
};

constexpr int kFarAway = 1 << 24;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct PairGeom {
    bool img_ok, win_ok;                    // the image lies inside the packed buffer; both windows lie inside the image
    int h, w, top[2], left[2];
    const unsigned char *img;
};

__device__ __forceinline__ PairGeom pair_geom(const SynthArgs &a, int p) {
    PairGeom g;
    g.h = a.sizes[2 * p];
    g.w = a.sizes[2 * p + 1];
    const long long off = a.offsets[p];
    g.img_ok = g.h > 0 && g.w > 0 && off >= 0 && (unsigned long long)off + (unsigned long long)g.h * g.w * 3 <= a.packed_bytes;
    g.img = a.packed + (g.img_ok ? off : 0);
    g.top[0] = a.win_src[2 * p];
    g.left[0] = a.win_src[2 * p + 1];
    g.top[1] = a.win_dst[2 * p];
    g.left[1] = a.win_dst[2 * p + 1];
    g.win_ok = g.img_ok;
    for (int s = 0; s < 2; ++s) {
        g.win_ok = g.win_ok && g.top[s] >= 0 && g.left[s] >= 0 && g.top[s] <= g.h - a.patch && g.left[s] <= g.w - a.patch;
        g.top[s] = clampi(g.top[s], -kFarAway, kFarAway);        // (a window far outside: no overflow in top + row below)
        g.left[s] = clampi(g.left[s], -kFarAway, kFarAway);
    }
    return g;
}

// the 8-bit value of channel c at (y, x), 0 outside the image
__device__ __forceinline__ int tap_u8(const PairGeom &g, int y, int x, int c) {
    return (y >= 0 && y < g.h && x >= 0 && x < g.w) ? (int)g.img[((long)y * g.w + x) * 3 + c] : 0;
}

// n (1..4) values of one row at out[0..n): one 16-byte store where the row layout allows it
__device__ __forceinline__ void store_px(float *out, const float (&v)[kImgPx], int n, int vec) {
    if (vec && n == kImgPx) {
        *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < n; ++j) out[j] = v[j];
    }
}

__global__ __launch_bounds__(kImgThreads) void synth_image_kernel(SynthArgs a) {
    __shared__ float s_norm[256];
    __shared__ double s_m[9];
    __shared__ int s_inv_ok;
    __shared__ int s_red[kImgThreads / 64];
    const int p = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
    s_norm[tid] = (float)((double)tid / 255.0);                  // (kImgThreads == 256: one entry per thread)
    const PairGeom g = pair_geom(a, p);
    if (side == 1 && tid == 0) {
        double ih[9], m[9];
        for (int k = 0; k < 9; ++k) ih[k] = a.inv_h[9 * (long)p + k];
        s_inv_ok = invert3(ih, m) ? 1 : 0;                       // cv2 inverts the matrix it is handed (no WARP_INVERSE_MAP)
        for (int k = 0; k < 9; ++k) s_m[k] = s_inv_ok ? m[k] : 0.0;
    }
    __syncthreads();

    const int patch = a.patch, qpr = (patch + kImgPx - 1) / kImgPx;
    const int q = blockIdx.x * kImgThreads + tid;                // (patch <= kMaxPatch: fits)
    int vmax = 0;
    if (q < qpr * patch) {
        const int row = q / qpr, x0 = (q - row * qpr) * kImgPx;
        const int n = patch - x0 < kImgPx ? patch - x0 : kImgPx;
        int v8[3][kImgPx] = {};
        if (g.img_ok && side == 0) {
            // (a window that leaves its image: clamped reads, never out of bounds)
            const int y = clampi(g.top[0] + row, 0, g.h - 1);
            for (int j = 0; j < n; ++j) {
                const int x = clampi(g.left[0] + x0 + j, 0, g.w - 1);
                const unsigned char *px = g.img + ((long)y * g.w + x) * 3;
                v8[0][j] = px[0];
                v8[1][j] = px[1];
                v8[2][j] = px[2];
            }
        } else if (g.img_ok && s_inv_ok) {
            const int y = g.top[1] + row;
            for (int j = 0; j < n; ++j) {
                int sx, sy, fx, fy;
                warp_source_q5(s_m, y, g.left[1] + x0 + j, &sx, &sy, &fx, &fy);
                const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32,
                          w11 = fx * fy * 32;
                // (a tap more than one pixel outside has all four reads refused by tap_u8; sx + 1 cannot overflow: |sx| < 2^26)
                for (int c = 0; c < 3; ++c) {
                    const int sum = tap_u8(g, sy, sx, c) * w00 + tap_u8(g, sy, sx + 1, c) * w01 + tap_u8(g, sy + 1, sx, c) * w10 +
                                    tap_u8(g, sy + 1, sx + 1, c) * w11;
                    v8[c][j] = (sum + 16384) >> 15;
                    vmax = v8[c][j] > vmax ? v8[c][j] : vmax;
                }
            }
        }
        const long pp = (long)patch * patch, at = (long)row * patch + x0;
        float *img = (side ? a.img_dst : a.img_src) + (long)p * 3 * pp + at;
        for (int c = 0; c < 3; ++c) {
            float v[kImgPx];
            for (int j = 0; j < kImgPx; ++j) v[j] = s_norm[v8[c][j]];
            store_px(img + c * pp, v, n, a.vec);
        }
        const float zero[kImgPx] = {0.0f, 0.0f, 0.0f, 0.0f};
        store_px((side ? a.heat_dst : a.heat_src) + (long)p * pp + at, zero, n, a.vec);
    }
    if (side == 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int t = __shfl_xor(vmax, o);
            vmax = t > vmax ? t : vmax;
        }
        if ((tid & 63) == 0) s_red[tid >> 6] = vmax;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kImgThreads / 64; ++w) vmax = s_red[w] > vmax ? s_red[w] : vmax;
            a.blk_max[(long)p * a.nblk + blockIdx.x] = vmax;
        }
    }
}

// order-preserving map of a float32 onto unsigned: a < b  <=>  key(a) < key(b); -0 counts as +0, as in a comparison
__device__ __forceinline__ unsigned prob_key32(float v) {
    const unsigned b = v == 0.0f ? 0u : __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kLblThreads) void synth_labels_kernel(SynthArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned s_hist[256];
    __shared__ int s_tmp[4];
    __shared__ int s_red[kLblThreads / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const PairGeom g = pair_geom(a, p);
    const int o0 = a.pts_off[p], o1 = a.pts_off[p + 1];
    const int n = (g.img_ok && o0 >= 0 && o1 >= o0 && o1 <= a.pts_total) ? o1 - o0 : 0;
    const float *pts = a.pts + 3 * (long)(n > 0 ? o0 : 0);

    // select_k_best: key > thr, or key == thr with index <= idx_cut (higher prob first, then the lower row index)
    unsigned thr = 0u;
    int idx_cut = 0x7fffffff;
    if (a.top_k > 0 && n > a.top_k) {
        int n_eq, need_eq;
        thr = (unsigned)radix_select<32, true, kLblThreads>(
            a.top_k,
            [&](auto count) {
                for (int i = tid; i < n; i += kLblThreads) count(prob_key32(pts[3 * (long)i + 2]));
            },
            s_hist, s_tmp, &n_eq, &need_eq);
        if (n_eq > need_eq) {
            int d0, d1;
            const unsigned t = thr;
            idx_cut = (int)radix_select<32, false, kLblThreads>(
                need_eq,
                [&](auto count) {
                    for (int i = tid; i < n; i += kLblThreads)
                        if (prob_key32(pts[3 * (long)i + 2]) == t) count((unsigned)i);
                },
                s_hist, s_tmp, &d0, &d1);
        }
    }

    float hm[9];
    for (int k = 0; k < 9; ++k) hm[k] = (float)a.inv_h[9 * (long)p + k];    // torch.tensor(inv_h, dtype=torch.float32)
    const int patch = a.patch;
    const long pp = (long)patch * patch;
    float *heat_src = a.heat_src + (long)p * pp, *heat_dst = a.heat_dst + (long)p * pp;
    const float x_max = (float)(g.w - 1), y_max = (float)(g.h - 1);
    for (int i = tid; i < n; i += kLblThreads) {
        const unsigned k = prob_key32(pts[3 * (long)i + 2]);
        if (!(k > thr || (k == thr && i <= idx_cut))) continue;
        const int xi = (int)pts[3 * (long)i], yi = (int)pts[3 * (long)i + 1];      // astype(int) / .long(): truncation
        const long r = (long)yi - g.top[0], c = (long)xi - g.left[0];
        if (r >= 0 && r < patch && c >= 0 && c < patch) heat_src[(long)r * patch + c] = 1.0f;
        const float fx = (float)xi, fy = (float)yi;
        const float xn = (hm[0] * fx + hm[1] * fy) + hm[2];
        const float yn = (hm[3] * fx + hm[4] * fy) + hm[5];
        const float zn = (hm[6] * fx + hm[7] * fy) + hm[8];
        const float xw = xn / zn, yw = yn / zn;
        if (xw >= 0.0f && xw <= x_max && yw >= 0.0f && yw <= y_max) {           // filter_points on the full image (NaN: dropped)
            const int rd = (int)rintf(yw) - g.top[1], cd = (int)rintf(xw) - g.left[1];
            if (rd >= 0 && rd < patch && cd >= 0 && cd < patch) heat_dst[(long)rd * patch + cd] = 1.0f;
        }
    }

    // dst_max: the largest 8-bit value of the destination patch; -1 for a pair that was not synthesised as asked
    int m = 0;
    for (int b = tid; b < a.nblk; b += kLblThreads) {
        const int v = a.blk_max[(long)p * a.nblk + b];
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    __syncthreads();                                             // (s_red is free: the selects have ended)
    if ((tid & 63) == 0) s_red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kLblThreads / 64; ++w) m = s_red[w] > m ? s_red[w] : m;
        a.dst_max[p] = g.win_ok ? m : -1;
    }
}

int image_blocks(int patch) {
    const long quads = (long)((patch + kImgPx - 1) / kImgPx) * patch;
    return balf_ceil_div(quads, kImgThreads);
}

bool sizes_ok(int P, int patch) { return P > 0 && P <= kMaxPairs && patch > 0 && patch <= kMaxPatch; }

// the workspace: blk_max [P, image_blocks(patch)], the destination image's maximum per workgroup of the image kernel
struct SynthWs { int *blk_max; size_t total; };
SynthWs synth_layout(int P, int patch, void *base = nullptr) {
    WorkspaceCursor c{static_cast<char *>(base), 0};
    int *blk_max = c.take<int>((size_t)P * image_blocks(patch) * sizeof(int));
    return {blk_max, c.used};
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_synth_pairs_workspace_bytes(int P, int patch) {
    if (!sizes_ok(P, patch)) return 0;
    return synth_layout(P, patch).total;
}

extern "C" int balf_synth_pairs(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                                const int32_t *sizes_dev, int P, const double *inv_h_dev, const int32_t *win_src_dev,
                                const int32_t *win_dst_dev, const float *pts_dev, int pts_total, const int32_t *pts_offsets_dev,
                                int top_k, int patch, float *img_src_dev, float *img_dst_dev, float *heat_src_dev,
                                float *heat_dst_dev, int32_t *dst_max_dev, void *workspace_dev, size_t workspace_bytes,
                                void *stream) {
    // (no label rows at all, pts_total == 0, may come with a null pts_dev: an empty tensor has none)
    if (!packed_dev || !offsets_dev || !sizes_dev || !inv_h_dev || !win_src_dev || !win_dst_dev || (!pts_dev && pts_total != 0) ||
        !pts_offsets_dev || !img_src_dev || !img_dst_dev || !heat_src_dev || !heat_dst_dev || !dst_max_dev || !workspace_dev)
        return BALF_ERR_ARG;
    if (P <= 0 || P > kMaxPairs || patch <= 0 || pts_total < 0 || top_k < 0) return BALF_ERR_ARG;
    if (patch > kMaxPatch) return BALF_ERR_SHAPE;
    const SynthWs ws = synth_layout(P, patch, workspace_dev);
    if (workspace_bytes < ws.total) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SynthArgs a{};
    a.packed = packed_dev;
    a.packed_bytes = packed_bytes;
    a.offsets = offsets_dev;
    a.sizes = sizes_dev;
    a.inv_h = inv_h_dev;
    a.win_src = win_src_dev;
    a.win_dst = win_dst_dev;
    a.pts = pts_dev;
    a.pts_off = pts_offsets_dev;
    a.pts_total = pts_total;
    a.top_k = top_k;
    a.patch = patch;
    a.nblk = image_blocks(patch);
    // 16-byte stores need rows of whole quads and 16-byte aligned planes
    a.vec = (patch % kImgPx == 0) && (((uintptr_t)img_src_dev | (uintptr_t)img_dst_dev | (uintptr_t)heat_src_dev |
                                       (uintptr_t)heat_dst_dev) & 15u) == 0;
    a.img_src = img_src_dev;
    a.img_dst = img_dst_dev;
    a.heat_src = heat_src_dev;
    a.heat_dst = heat_dst_dev;
    a.dst_max = dst_max_dev;
    a.blk_max = ws.blk_max;
    synth_image_kernel<<<dim3(a.nblk, 2, P), kImgThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    synth_labels_kernel<<<P, kLblThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
