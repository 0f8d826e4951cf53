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
//   balf_synth_train_pairs   the TRAINING task's pairs (COCO.py:70-75, task == 'train'): the same two launches, the image kernel
//     in its training form (synth_image_kernel<true>): the destination patch is the warp of bgr_photometric_to_rgb(image), and
//     the distorted image is never formed: each of the four taps of an output pixel is distorted, all three channels, before
//     the integer interpolation; a tap outside the image contributes 0 (the reference pads the DISTORTED image with zeros).
//     Side-1 workgroups build the pair's PhotoTables in LDS (3 KiB) before the barrier they already have.
//   balf_photometric_u8      bgr_distorsion (dataset_utils.py:81-121) of whole packed images with given parameters: one launch,
//     photometric_kernel     grid (blocks, B), 256 threads, four pixels (12 bytes, three dwords where the image is 4-byte aligned)
//                            per thread and step of a grid-stride loop.
//   photo_distort            the ONE distortion function of both kernels.  The value maps that depend on the pair's float64
//                            parameters (brightness + first contrast, saturation, hue, second contrast) and OpenCV's sdiv /
//                            hdiv tables are 256-entry LDS tables (PhotoTables, one entry per thread: the float64 work happens
//                            there and nowhere else); per pixel the rest is integer arithmetic and the float32 HSV -> BGR of
//                            OpenCV's scalar 8-bit code, fp contraction off.  Every table index is a byte read from a table or
//                            from the image, so no index leaves its table whatever bits the parameters hold.
//                            The two conversions are DEFINED by that scalar code (include/balf_hip.h); cv2 parity is UNPINNED.
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
    const double *photo;                    // [P, 5] (delta_b, alpha1, sat, hue, alpha2); balf_synth_train_pairs only, else null
    const int *perm;                        // [P] row of kPerms; null with photo
};

constexpr int kFarAway = 1 << 24;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the photometric distortion of the training task (dataset_utils.py:76-121) ----------------------------------------------
constexpr int kNumPerms = 6;
// the reference's perms, row r in bits 6r .. 6r + 5, two bits per entry: out_bgr[k] = bgr[perms[r][k]]
constexpr unsigned long long perm_row(int a, int b, int c) { return (unsigned long long)(a | (b << 2) | (c << 4)); }
constexpr unsigned long long kPerms = perm_row(0, 1, 2) | perm_row(0, 2, 1) << 6 | perm_row(1, 0, 2) << 12 | perm_row(1, 2, 0) << 18 |
                                      perm_row(2, 0, 1) << 24 | perm_row(2, 1, 0) << 30;
constexpr int kPhotoThreads = 256;          // one table entry per thread: both kernels that distort run 256 threads

struct PhotoTables {
    int sdiv[256], hdiv[256];               // OpenCV's RGB2HSV_b tables, hrange 180, hsv_shift 12
    unsigned char pre[256], sat[256], hue[256], post[256];      // steps 1, 3, 4 and 6 of include/balf_hip.h as byte -> byte maps
};

__device__ __forceinline__ double clamp255(double x) {           // check_margins: two comparisons, a NaN passes
    x = x > 255.0 ? 255.0 : x;
    return x < 0.0 ? 0.0 : x;
}

// entry i of every table from prm = (delta_b, alpha1, sat, hue, alpha2); the caller's barrier publishes them
__device__ __forceinline__ void photo_build(PhotoTables &t, const double *prm, int i) {
#pragma clang fp contract(off)
    const double x = (double)i;
    t.sdiv[i] = i ? (int)rint((double)(255 << 12) / x) : 0;
    t.hdiv[i] = i ? (int)rint((double)(180 << 12) / (6.0 * x)) : 0;
    t.pre[i] = (unsigned char)(int)clamp255(clamp255(x + prm[0]) * prm[1]);
    t.sat[i] = (unsigned char)(int)clamp255(x * prm[2]);
    double h = x + prm[3];
    h = h > 360.0 ? h - 360.0 : h;
    h = h < 0.0 ? h + 360.0 : h;
    t.hue[i] = (unsigned char)((int)h & 255);                    // astype(np.uint8) of 324..359: 68..103, as the reference
    t.post[i] = (unsigned char)(int)clamp255(x * prm[4]);
}

__device__ __forceinline__ int sel3(int i, int v0, int v1, int v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }

// rint(x * 255.f) saturated to a byte (saturate_cast<uchar>: half to even)
__device__ __forceinline__ int to_u8(float x) {
#pragma clang fp contract(off)
    const float y = __builtin_rintf(x * 255.0f);
    return y < 0.0f ? 0 : (y > 255.0f ? 255 : (int)y);
}

// one pixel through steps 1-7; perm_bits = the six bits of the pair's row of kPerms
__device__ __forceinline__ void photo_distort(const PhotoTables &t, unsigned perm_bits, int &b, int &g, int &r) {
#pragma clang fp contract(off)
    b = t.pre[b];
    g = t.pre[g];
    r = t.pre[r];
    // RGB2HSV_b
    int v = b > g ? b : g, vmin = b < g ? b : g;
    v = r > v ? r : v;
    vmin = r < vmin ? r : vmin;
    const int diff = v - vmin;
    const int s0 = (diff * t.sdiv[v] + (1 << 11)) >> 12;
    const int h0 = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    int hq = (h0 * t.hdiv[diff] + (1 << 11)) >> 12;
    hq += hq < 0 ? 180 : 0;
    const int S = t.sat[s0 & 255], H = t.hue[hq & 255];          // (s0 <= 255 and 0 <= hq < 180 already: the masks cost nothing)
    // HSV2RGB_b: OpenCV's float32 path
    const float s = (float)S * (1.0f / 255.0f), vv = (float)v * (1.0f / 255.0f);
    float fb = vv, fg = vv, fr = vv;
    if (S != 0) {
        float hh = (float)H * (6.0f / 180.0f);
        hh = hh >= 6.0f ? hh - 6.0f : hh;                         // (H <= 255: hh < 9, once is enough)
        int sector = (int)hh;                                    // floor: hh >= 0
        const float f = hh - (float)sector;
        sector = sector > 5 ? 5 : sector;
        const float tab1 = vv * (1.0f - s), tab2 = vv * (1.0f - s * f), tab3 = vv * (1.0f - s * (1.0f - f));
        // sector_data: {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0} -> (b, g, r)
        fb = sector == 0 || sector == 1 ? tab1 : (sector == 2 ? tab3 : (sector == 5 ? tab2 : vv));
        fg = sector == 0 ? tab3 : (sector == 1 || sector == 2 ? vv : (sector == 3 ? tab2 : tab1));
        fr = sector == 0 || sector == 5 ? vv : (sector == 1 ? tab2 : (sector == 4 ? tab3 : tab1));
    }
    const int pb = t.post[to_u8(fb)], pg = t.post[to_u8(fg)], pr = t.post[to_u8(fr)];
    b = sel3(perm_bits & 3, pb, pg, pr);
    g = sel3((perm_bits >> 2) & 3, pb, pg, pr);
    r = sel3((perm_bits >> 4) & 3, pb, pg, pr);
}

struct PairGeom {
    bool img_ok, win_ok;                    // the image lies inside the packed buffer; both windows lie inside the image (and, in
                                            // the training form, perm names a row of kPerms): the pair is synthesised as asked
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
    if (a.perm) g.win_ok = g.win_ok && (unsigned)a.perm[p] < (unsigned)kNumPerms;
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

template <bool kTrain> struct PhotoLds {};                       // the tables take LDS in the training form only
template <> struct PhotoLds<true> { PhotoTables t; };

// the three channels of the pixel at (y, x) as the training task sees them, in the packed image's R, G, B order: distorted
// (the packed images are RGB: blue is px[2]), all 0 outside the image -- NOT the distortion of a black pixel
__device__ __forceinline__ void tap_photo(const PairGeom &g, const PhotoTables &t, unsigned perm_bits, int y, int x, int (&v)[3]) {
    v[0] = v[1] = v[2] = 0;
    if (y >= 0 && y < g.h && x >= 0 && x < g.w) {
        const unsigned char *px = g.img + ((long)y * g.w + x) * 3;
        int b = px[2], gr = px[1], r = px[0];
        photo_distort(t, perm_bits, b, gr, r);
        v[0] = r;
        v[1] = gr;
        v[2] = b;
    }
}

// kTrain: the destination side warps the photometrically distorted image (balf_synth_train_pairs); everything else is shared
template <bool kTrain>
__global__ __launch_bounds__(kImgThreads) void synth_image_kernel(SynthArgs a) {
    static_assert(kImgThreads == kPhotoThreads, "one table entry per thread");
    __shared__ float s_norm[256];
    __shared__ double s_m[9];
    __shared__ int s_inv_ok;
    __shared__ int s_red[kImgThreads / 64];
    __shared__ PhotoLds<kTrain> s_photo;
    const int p = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
    s_norm[tid] = (float)((double)tid / 255.0);                  // (kImgThreads == 256: one entry per thread)
    const PairGeom g = pair_geom(a, p);
    unsigned perm_bits = 0;
    bool perm_ok = true;
    if constexpr (kTrain) {
        if (side == 1) {
            photo_build(s_photo.t, a.photo + 5 * (long)p, tid);
            const int pm = a.perm[p];
            perm_ok = (unsigned)pm < (unsigned)kNumPerms;
            perm_bits = perm_ok ? (unsigned)(kPerms >> (6 * pm)) & 63u : 0u;
        }
    }
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
        } else if (g.img_ok && s_inv_ok && perm_ok) {
            const int y = g.top[1] + row;
            for (int j = 0; j < n; ++j) {
                int sx, sy, fx, fy;
                warp_source_q5(s_m, y, g.left[1] + x0 + j, &sx, &sy, &fx, &fy);
                const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32,
                          w11 = fx * fy * 32;
                // (a tap more than one pixel outside has all four reads refused by tap_u8; sx + 1 cannot overflow: |sx| < 2^26)
                if constexpr (kTrain) {
                    int t00[3], t01[3], t10[3], t11[3];
                    tap_photo(g, s_photo.t, perm_bits, sy, sx, t00);
                    tap_photo(g, s_photo.t, perm_bits, sy, sx + 1, t01);
                    tap_photo(g, s_photo.t, perm_bits, sy + 1, sx, t10);
                    tap_photo(g, s_photo.t, perm_bits, sy + 1, sx + 1, t11);
                    for (int c = 0; c < 3; ++c) {
                        const int sum = t00[c] * w00 + t01[c] * w01 + t10[c] * w10 + t11[c] * w11;
                        v8[c][j] = (sum + 16384) >> 15;
                        vmax = v8[c][j] > vmax ? v8[c][j] : vmax;
                    }
                } else {
                    for (int c = 0; c < 3; ++c) {
                        const int sum = tap_u8(g, sy, sx, c) * w00 + tap_u8(g, sy, sx + 1, c) * w01 +
                                        tap_u8(g, sy + 1, sx, c) * w10 + tap_u8(g, sy + 1, sx + 1, c) * w11;
                        v8[c][j] = (sum + 16384) >> 15;
                        vmax = v8[c][j] > vmax ? v8[c][j] : vmax;
                    }
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

// ---- balf_photometric_u8: whole images --------------------------------------------------------------------------------------
constexpr int kPhotoPx = 4;                 // pixels per thread and step: 12 bytes, three dwords
constexpr int kPhotoMaxBlocks = 4096;

struct PhotoArgs {
    const unsigned char *packed;
    size_t packed_bytes;
    const long long *offsets;               // [B]
    const int *sizes;                       // [B, 2] (h, w)
    const double *params;                   // [B, 5]
    const int *perm;                        // [B]
    int blue_idx;                           // 0: the pixels are B, G, R; 2: R, G, B
    unsigned char *out;
};

__global__ __launch_bounds__(kPhotoThreads) void photometric_kernel(PhotoArgs a) {
    __shared__ PhotoTables s_t;
    const int b = blockIdx.y, tid = threadIdx.x;
    photo_build(s_t, a.params + 5 * (long)b, tid);
    __syncthreads();
    const int h = a.sizes[2 * b], w = a.sizes[2 * b + 1];
    const long long off = a.offsets[b];
    // (h * w <= 2^62: the product by 3 is formed only once it is known to be small)
    if (h <= 0 || w <= 0 || off < 0 || (unsigned long long)off > a.packed_bytes) return;
    const unsigned long long npx = (unsigned long long)h * (unsigned long long)w;
    if (npx > (a.packed_bytes - (unsigned long long)off) / 3) return;                 // the image leaves the buffer: not written
    const int pm = a.perm[b];
    const bool perm_ok = (unsigned)pm < (unsigned)kNumPerms;
    const unsigned perm_bits = perm_ok ? (unsigned)(kPerms >> (6 * pm)) & 63u : 0u;
    const unsigned char *in = a.packed + off;
    unsigned char *out = a.out + off;
    const bool dwords = (((uintptr_t)in | (uintptr_t)out) & 3u) == 0;
    const int bi = a.blue_idx;
    const unsigned long long groups = (npx + kPhotoPx - 1) / kPhotoPx;
    for (unsigned long long q = (unsigned long long)blockIdx.x * kPhotoThreads + tid; q < groups;
         q += (unsigned long long)gridDim.x * kPhotoThreads) {
        const unsigned long long px0 = q * kPhotoPx;
        const int n = npx - px0 < (unsigned long long)kPhotoPx ? (int)(npx - px0) : kPhotoPx;
        const bool whole = dwords && n == kPhotoPx;
        unsigned char v[3 * kPhotoPx] = {};
        if (whole) {
            const uint3 d = *reinterpret_cast<const uint3 *>(in + 3 * px0);          // 12-byte groups of a 4-byte aligned image
            const unsigned dw[3] = {d.x, d.y, d.z};
            for (int k = 0; k < 3 * kPhotoPx; ++k) v[k] = (unsigned char)(dw[k >> 2] >> (8 * (k & 3)));
        } else {
            for (int k = 0; k < 3 * n; ++k) v[k] = in[3 * px0 + k];
        }
        for (int j = 0; j < kPhotoPx; ++j) {
            int cb = v[3 * j + bi], cg = v[3 * j + 1], cr = v[3 * j + 2 - bi];
            photo_distort(s_t, perm_bits, cb, cg, cr);
            v[3 * j + bi] = (unsigned char)(perm_ok ? cb : 0);                        // a perm outside the table: a black image
            v[3 * j + 1] = (unsigned char)(perm_ok ? cg : 0);
            v[3 * j + 2 - bi] = (unsigned char)(perm_ok ? cr : 0);
        }
        if (whole) {
            unsigned dw[3] = {0u, 0u, 0u};
            for (int k = 0; k < 3 * kPhotoPx; ++k) dw[k >> 2] |= (unsigned)v[k] << (8 * (k & 3));
            *reinterpret_cast<uint3 *>(out + 3 * px0) = make_uint3(dw[0], dw[1], dw[2]);
        } else {
            for (int k = 0; k < 3 * n; ++k) out[3 * px0 + k] = v[k];
        }
    }
}

// both pair entries: photo_dev / perm_dev null = the validation task
int synth_pairs_launch(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev, const int32_t *sizes_dev,
                       int P, const double *inv_h_dev, const int32_t *win_src_dev, const int32_t *win_dst_dev, const float *pts_dev,
                       int pts_total, const int32_t *pts_offsets_dev, int top_k, int patch, float *img_src_dev, float *img_dst_dev,
                       float *heat_src_dev, float *heat_dst_dev, int32_t *dst_max_dev, void *workspace_dev, size_t workspace_bytes,
                       const double *photo_dev, const int32_t *perm_dev, void *stream) {
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
    a.photo = photo_dev;
    a.perm = perm_dev;
    if (photo_dev)
        synth_image_kernel<true><<<dim3(a.nblk, 2, P), kImgThreads, 0, st>>>(a);
    else
        synth_image_kernel<false><<<dim3(a.nblk, 2, P), kImgThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    synth_labels_kernel<<<P, kLblThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
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
    return synth_pairs_launch(packed_dev, packed_bytes, offsets_dev, sizes_dev, P, inv_h_dev, win_src_dev, win_dst_dev, pts_dev,
                              pts_total, pts_offsets_dev, top_k, patch, img_src_dev, img_dst_dev, heat_src_dev, heat_dst_dev,
                              dst_max_dev, workspace_dev, workspace_bytes, nullptr, nullptr, stream);
}

extern "C" int balf_synth_train_pairs(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                                      const int32_t *sizes_dev, int P, const double *inv_h_dev, const int32_t *win_src_dev,
                                      const int32_t *win_dst_dev, const float *pts_dev, int pts_total,
                                      const int32_t *pts_offsets_dev, int top_k, int patch, float *img_src_dev, float *img_dst_dev,
                                      float *heat_src_dev, float *heat_dst_dev, int32_t *dst_max_dev, void *workspace_dev,
                                      size_t workspace_bytes, const double *params_dev, const int32_t *perm_dev, void *stream) {
    if (!params_dev || !perm_dev) return BALF_ERR_ARG;
    return synth_pairs_launch(packed_dev, packed_bytes, offsets_dev, sizes_dev, P, inv_h_dev, win_src_dev, win_dst_dev, pts_dev,
                              pts_total, pts_offsets_dev, top_k, patch, img_src_dev, img_dst_dev, heat_src_dev, heat_dst_dev,
                              dst_max_dev, workspace_dev, workspace_bytes, params_dev, perm_dev, stream);
}

extern "C" int balf_photometric_u8(const unsigned char *packed_dev, size_t packed_bytes, const long long *offsets_dev,
                                   const int32_t *sizes_dev, int B, const double *params_dev, const int32_t *perm_dev, int blue_idx,
                                   unsigned char *out_dev, void *stream) {
    if (!packed_dev || !offsets_dev || !sizes_dev || !params_dev || !perm_dev || !out_dev) return BALF_ERR_ARG;
    if (B <= 0 || B > kMaxPairs || (blue_idx != 0 && blue_idx != 2)) return BALF_ERR_ARG;
    PhotoArgs a{packed_dev, packed_bytes, offsets_dev, sizes_dev, params_dev, perm_dev, blue_idx, out_dev};
    // the sizes live on the device: twice the blocks an image of the average size needs, the grid-stride loop takes the rest
    const size_t per_block = (size_t)3 * kPhotoPx * kPhotoThreads;
    size_t blocks = 2 * ((packed_bytes / (size_t)B + per_block) / per_block);
    blocks = blocks > (size_t)kPhotoMaxBlocks ? (size_t)kPhotoMaxBlocks : blocks;
    photometric_kernel<<<dim3((unsigned)blocks, B), kPhotoThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
