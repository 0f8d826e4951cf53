// Multi-scale keypoint extraction over an image pyramid, gfx950 (multi-scale extraction).
//
// The HSequences extraction protocol that balf/configs/config_hpatches.py:50-80 configures
// (scale_factor_levels, pyramid_levels, upsampled_levels, num_points, nms_size, border_size) and whose point format
// get_point_coordinates(..., scale_value, order_coord) and apply_homography_to_points carry.  The reference ships no
// driver for it; balf_amd/multiscale.py states the protocol and drives these kernels:
//   pyramid_level_kernel  one 8 x 64 output tile of one level per workgroup: the source footprint of the tile plus the
//                         blur halo -> LDS (half-sample symmetric border), separable Gaussian (row pass, column pass) in
//                         LDS, bilinear resample with half-pixel centres, written straight into the zero-padded NCHW fp32
//                         batch balf_forward takes (padding included: every padded pixel is written, 0 outside the image)
//   (budgeted top-K)      balf_nms_topk_budget: the kernels of balf_nms_topk (nms_topk.hip) with K decided per image
//   merge_kernel          one workgroup per image: the L level lists -> LDS keys (score desc, level asc, index asc),
//                         bitonic sort (block_ops.h), each row mapped to the original image with the homography arithmetic
//                         of balf_apply_homography (homography.h), [N,4] float64 rows + count
#include <cmath>
#include <cstdint>

#include "block_ops.h"
#include "common.h"
#include "homography.h"
#include "prof.h"

namespace {

constexpr int PYR_THREADS = 256;
constexpr int PYR_TX = 64;                 // output tile width (a wave's worth of consecutive pixels per row)
constexpr int PYR_LDS_MAX = 64 * 1024;     // bytes for the two staging planes

struct PyrArgs {
    const void *src;
    int kind;                  // BALF_PYR_SRC_*
    int gray;                  // one distinct channel: computed once, written to the three planes
    int h_in, w_in;
    long s_b, s_c, s_y, s_x;   // element strides of the source
    long s_off;                // element offset of image 0, channel 0, pixel (0, 0)
    int h_out, w_out, hp, wp, top, left;
    double sc_y, sc_x;         // in / out
    int R;                     // blur radius (0: no blur)
    float taps[2 * BALF_PYR_MAX_RADIUS + 1];
    int ty, fh, fw;            // tile height, LDS footprint (rows, columns)
    float *dst;                // [B,3,hp,wp]
};

// scipy.ndimage mode='reflect' (half-sample symmetric) for any offset
__device__ __forceinline__ int reflect(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// F.interpolate(bilinear, align_corners=False) source coordinate: (o + 0.5) * in/out - 0.5, clamped below at 0; float64 so
// that the position of a pixel far into a large level carries no fp32 rounding (2.4e-4 pixel at x ~ 3800)
__device__ __forceinline__ void src_coord(int o, double sc, int n_in, int *i0, int *i1, float *lam) {
    double s = ((double)o + 0.5) * sc - 0.5;
    s = s < 0.0 ? 0.0 : s;
    int i = (int)s;
    if (i > n_in - 1) i = n_in - 1;
    *i0 = i;
    *i1 = i < n_in - 1 ? i + 1 : i;
    *lam = (float)(s - (double)i);
}

__device__ __forceinline__ float load_src(const PyrArgs &a, int b, int c, int y, int x) {
    const long o = a.s_off + (long)b * a.s_b + (long)c * a.s_c + (long)y * a.s_y + (long)x * a.s_x;
    if (a.kind == BALF_PYR_SRC_U8) return (float)((double)static_cast<const unsigned char *>(a.src)[o] / 255.0);
    return static_cast<const float *>(a.src)[o];
}

__global__ __launch_bounds__(PYR_THREADS) void pyramid_level_kernel(PyrArgs a) {
    extern __shared__ float lds[];
    float *S = lds;                            // [fh][fw] raw footprint, then the blurred plane
    float *Hb = lds + a.fh * a.fw;             // [fh][fw] row-blurred
    const int b = blockIdx.z;
    const int py0 = blockIdx.y * a.ty, px0 = blockIdx.x * PYR_TX;
    const int tid = threadIdx.x;
    const long plane = (long)a.hp * a.wp;
    float *dst = a.dst + (long)b * 3 * plane;
    // the tile's image rows / columns
    const int iy_lo = max(py0 - a.top, 0), iy_hi = min(py0 + a.ty - a.top, a.h_out);       // [lo, hi)
    const int ix_lo = max(px0 - a.left, 0), ix_hi = min(px0 + PYR_TX - a.left, a.w_out);
    const int n_out = a.ty * PYR_TX;
    if (iy_lo >= iy_hi || ix_lo >= ix_hi) {    // padding only
        for (int t = tid; t < n_out; t += PYR_THREADS) {
            const int py = py0 + t / PYR_TX, px = px0 + t % PYR_TX;
            if (py < a.hp && px < a.wp)
                for (int c = 0; c < 3; ++c) dst[c * plane + (long)py * a.wp + px] = 0.0f;
        }
        return;
    }
    int sy_lo, sy_hi, sx_lo, sx_hi, d;
    float dl;
    src_coord(iy_lo, a.sc_y, a.h_in, &sy_lo, &d, &dl);
    src_coord(iy_hi - 1, a.sc_y, a.h_in, &d, &sy_hi, &dl);
    src_coord(ix_lo, a.sc_x, a.w_in, &sx_lo, &d, &dl);
    src_coord(ix_hi - 1, a.sc_x, a.w_in, &d, &sx_hi, &dl);
    const int R = a.R;
    const int nr = min(sy_hi - sy_lo + 1 + 2 * R, a.fh), nc = min(sx_hi - sx_lo + 1 + 2 * R, a.fw);   // (host bound: never cut)
    const int y_base = sy_lo - R, x_base = sx_lo - R;
    const int n_ch = a.gray ? 1 : 3;
    for (int c = 0; c < n_ch; ++c) {
        for (int t = tid; t < nr * nc; t += PYR_THREADS) {
            const int r = t / nc, q = t % nc;
            S[r * a.fw + q] = load_src(a, b, c, reflect(y_base + r, a.h_in), reflect(x_base + q, a.w_in));
        }
        __syncthreads();
        if (R > 0) {
            const int ncb = nc - 2 * R, nrb = nr - 2 * R;
            for (int t = tid; t < nr * ncb; t += PYR_THREADS) {
                const int r = t / ncb, q = t % ncb;
                const float *row = S + r * a.fw + q;
                float acc = 0.0f;
                for (int k = 0; k <= 2 * R; ++k) acc += a.taps[k] * row[k];
                Hb[r * a.fw + q] = acc;
            }
            __syncthreads();
            for (int t = tid; t < nrb * ncb; t += PYR_THREADS) {
                const int r = t / ncb, q = t % ncb;
                const float *col = Hb + r * a.fw + q;
                float acc = 0.0f;
                for (int k = 0; k <= 2 * R; ++k) acc += a.taps[k] * col[k * a.fw];
                S[r * a.fw + q] = acc;       // blurred pixel (sy_lo + r, sx_lo + q)
            }
            __syncthreads();
        }
        // with R = 0 the raw plane already starts at (sy_lo, sx_lo)
        for (int t = tid; t < n_out; t += PYR_THREADS) {
            const int py = py0 + t / PYR_TX, px = px0 + t % PYR_TX;
            if (py >= a.hp || px >= a.wp) continue;
            const int iy = py - a.top, ix = px - a.left;
            float v = 0.0f;
            if (iy >= 0 && iy < a.h_out && ix >= 0 && ix < a.w_out) {
                int y0, y1, x0, x1;
                float ly, lx;
                src_coord(iy, a.sc_y, a.h_in, &y0, &y1, &ly);
                src_coord(ix, a.sc_x, a.w_in, &x0, &x1, &lx);
                y0 -= sy_lo; y1 -= sy_lo; x0 -= sx_lo; x1 -= sx_lo;
                const float v00 = S[y0 * a.fw + x0], v01 = S[y0 * a.fw + x1];
                const float v10 = S[y1 * a.fw + x0], v11 = S[y1 * a.fw + x1];
                v = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
            }
            const long o = (long)py * a.wp + px;
            if (a.gray) {
                dst[o] = v; dst[plane + o] = v; dst[2 * plane + o] = v;
            } else {
                dst[c * plane + o] = v;
            }
        }
        __syncthreads();                       // the next channel reuses the LDS planes
    }
}

// make_shape_even + mod_padding_symmetric(64) (balf_amd/arch.py: padded_hw)
void padded_hw(int h, int w, int *hp, int *wp, int *top, int *left) {
    const int he = h + (h & 1), we = w + (w & 1);
    *hp = (he + 63) / 64 * 64;
    *wp = (we + 63) / 64 * 64;
    *top = *hp / 2 - he / 2;
    *left = *wp / 2 - we / 2;
}

// ---------------------------------------------------------------------------------------------
// merge of the level lists: one 1024-thread workgroup per image
// ---------------------------------------------------------------------------------------------
constexpr int MERGE_THREADS = 1024;
constexpr int LEVEL_BITS = 26;             // key low word: level << 26 | flat index (a level has < 2^25 padded pixels)

struct MergeLevel {
    double h[9];
    int w;
};
struct MergeArgs {
    const int32_t *idx, *cnt;                  // [L,B,K_max], [L,B]
    const float *score;                        // [L,B,K_max]
    int L, B, K_max, N, cap, npow2_cap, order_yx;
    double *pts;                               // [B,N,4]
    int32_t *count_out;                        // [B]
    MergeLevel lv[BALF_MAX_PYRAMID_LEVELS];
};

__global__ __launch_bounds__(MERGE_THREADS) void merge_kernel(MergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);      // [npow2_cap]
    __shared__ int s_off[BALF_MAX_PYRAMID_LEVELS + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int o = 0;
        for (int l = 0; l < a.L; ++l) {
            s_off[l] = o;
            o += balf::clamp_count(a.cnt, (long)l * a.B + b, a.K_max);
        }
        s_off[a.L] = o;
    }
    __syncthreads();
    const int total = s_off[a.L];
    double *out = a.pts + (long)b * a.N * 4;
    if (total > a.cap) {                       // cannot happen with budgeted lists (they sum to <= N): reported, not cut
        for (int i = tid; i < a.N * 4; i += MERGE_THREADS) out[i] = 0.0;
        if (tid == 0) a.count_out[b] = -1;
        return;
    }
    const int npow2 = balf::next_pow2(total);
    for (int p = tid; p < npow2; p += MERGE_THREADS) {
        unsigned long long k = ~0ull;
        if (p < total) {
            int l = 0;
            while (s_off[l + 1] <= p) ++l;
            const long e = ((long)l * a.B + b) * a.K_max + (p - s_off[l]);
            const unsigned sb = __float_as_uint(a.score[e]);
            k = ((unsigned long long)(~sb) << 32) | ((unsigned)l << LEVEL_BITS) |
                ((unsigned)a.idx[e] & ((1u << LEVEL_BITS) - 1u));
        }
        keys[p] = k;                           // ascending = score desc, level asc, index asc
    }
    __syncthreads();
    balf::bitonic_sort<MERGE_THREADS>(keys, npow2);
    const int n = total < a.N ? total : a.N;
    for (int r = tid; r < a.N; r += MERGE_THREADS) {
        double *row = out + (long)r * 4;
        if (r >= n) {
            row[0] = 0.0; row[1] = 0.0; row[2] = 0.0; row[3] = 0.0;
            continue;
        }
        const unsigned long long kv = keys[r];
        const unsigned lo = (unsigned)(kv & 0xffffffffull);
        const int l = (int)(lo >> LEVEL_BITS), idx = (int)(lo & ((1u << LEVEL_BITS) - 1u));
        const float score = __uint_as_float(~(unsigned)(kv >> 32));
        const int w = a.lv[l].w;
        double x, y, rad;
        balf::homography_point(a.lv[l].h, (double)(idx % w), (double)(idx / w), 1.0, &x, &y, &rad);
        row[0] = a.order_yx ? y : x;
        row[1] = a.order_yx ? x : y;
        row[2] = rad;
        row[3] = (double)score;
    }
    if (tid == 0) a.count_out[b] = n;
}

}  // namespace

extern "C" int balf_pyramid_level(const void *src_dev, int src_kind, int channels, int B, int H_in, int W_in, double sigma,
                                  int H_out, int W_out, float *dst_dev, void *stream) {
    if (!src_dev || !dst_dev || B <= 0 || H_in <= 0 || W_in <= 0 || H_out <= 0 || W_out <= 0) return BALF_ERR_ARG;
    if (channels != 1 && channels != 3) return BALF_ERR_ARG;
    if (src_kind != BALF_PYR_SRC_U8 && src_kind != BALF_PYR_SRC_F32 && src_kind != BALF_PYR_SRC_LEVEL) return BALF_ERR_ARG;
    if (src_kind == BALF_PYR_SRC_F32 && channels != 3) return BALF_ERR_ARG;
    if (!(sigma < 64.0)) return BALF_ERR_ARG;                                     // (also rejects NaN)
    const int R = sigma > 0.0 ? (int)(4.0 * sigma + 0.5) : 0;                     // scipy: truncate = 4.0
    if (R > BALF_PYR_MAX_RADIUS) return BALF_ERR_ARG;
    PyrArgs a{};
    a.src = src_dev;
    a.kind = src_kind;
    a.gray = channels == 1;
    a.h_in = H_in;
    a.w_in = W_in;
    if (src_kind == BALF_PYR_SRC_LEVEL) {      // [B,3,Hp,Wp], image at (top, left); a gray level's three planes are equal
        int hp, wp, top, left;
        padded_hw(H_in, W_in, &hp, &wp, &top, &left);
        if ((long)hp * wp > (1L << 25)) return BALF_ERR_SHAPE;
        a.s_x = 1; a.s_y = wp; a.s_c = (long)hp * wp; a.s_b = 3L * hp * wp; a.s_off = (long)top * wp + left;
    } else {                                   // [B,H,W,channels]
        a.s_x = channels; a.s_y = (long)W_in * channels; a.s_c = channels == 3 ? 1 : 0; a.s_b = (long)H_in * W_in * channels;
        a.s_off = 0;
    }
    padded_hw(H_out, W_out, &a.hp, &a.wp, &a.top, &a.left);
    if ((long)a.hp * a.wp > (1L << 25)) return BALF_ERR_SHAPE;
    a.h_out = H_out;
    a.w_out = W_out;
    a.sc_y = (double)H_in / (double)H_out;
    a.sc_x = (double)W_in / (double)W_out;
    a.R = R;
    if (R > 0) {                               // exp(-k^2 / 2 sigma^2), normalised to sum 1 (gaussian_filter1d's taps)
        double t[2 * BALF_PYR_MAX_RADIUS + 1], sum = 0.0;
        for (int k = -R; k <= R; ++k) sum += (t[k + R] = exp(-0.5 * (double)k * k / (sigma * sigma)));
        for (int k = 0; k <= 2 * R; ++k) a.taps[k] = (float)(t[k] / sum);
    }
    // LDS footprint of a tile: the source rows/columns its outputs sample (<= ceil((T - 1) * in/out) + 2, +1 for rounding)
    // plus the blur halo on both sides; tiles shrink from 8 rows until two planes fit
    const int fw = (int)std::ceil((PYR_TX - 1) * a.sc_x) + 3 + 2 * R;
    int ty = 8, fh = 0;
    for (; ty >= 1; ty >>= 1) {
        fh = (int)std::ceil((ty - 1) * a.sc_y) + 3 + 2 * R;
        if ((size_t)2 * fh * fw * sizeof(float) <= PYR_LDS_MAX) break;
    }
    // even a one-row tile does not fit: fw > 65536 / (8 (3 + 2R)), i.e. a reduction factor along x of more than
    // ~43.28 without blur (R = 0: ceil(63 in/out) > 2727) down to ~6.54 at R = 8 (ceil(63 in/out) > 412)
    if (ty < 1) return BALF_ERR_ARG;
    a.ty = ty; a.fh = fh; a.fw = fw;
    a.dst = dst_dev;
    const size_t smem = (size_t)2 * fh * fw * sizeof(float);
    if (!balf_allow_dynamic_lds<pyramid_level_kernel>((int)smem)) return BALF_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    BALF_PROF(balf_prof::kMsPyramid, st,
              hipLaunchKernelGGL(pyramid_level_kernel, dim3(balf_ceil_div(a.wp, PYR_TX), balf_ceil_div(a.hp, ty), B),
                                 dim3(PYR_THREADS), smem, st, a));
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_multiscale_merge(const int32_t *idx_dev, const float *score_dev, const int32_t *count_dev, int L, int B,
                                     int K_max, const int32_t *level_w_host, const double *h_host, int N, int order_yx,
                                     double *pts_dev, int32_t *count_out_dev, void *stream) {
    if (!idx_dev || !score_dev || !count_dev || !level_w_host || !h_host || !pts_dev || !count_out_dev) return BALF_ERR_ARG;
    if (L <= 0 || L > BALF_MAX_PYRAMID_LEVELS || B <= 0 || K_max <= 0 || K_max > BALF_MAX_TOPK) return BALF_ERR_ARG;
    if (N <= 0 || N > BALF_MAX_TOPK) return BALF_ERR_ARG;
    MergeArgs a{};
    a.idx = idx_dev; a.score = score_dev; a.cnt = count_dev;
    a.L = L; a.B = B; a.K_max = K_max; a.N = N; a.order_yx = order_yx ? 1 : 0;
    a.pts = pts_dev; a.count_out = count_out_dev;
    for (int l = 0; l < L; ++l) {
        if (level_w_host[l] <= 0) return BALF_ERR_ARG;
        a.lv[l].w = level_w_host[l];
        for (int k = 0; k < 9; ++k) a.lv[l].h[k] = h_host[9 * l + k];
    }
    const long all = (long)L * K_max;
    a.cap = (int)(all < BALF_MAX_TOPK ? all : BALF_MAX_TOPK);
    a.npow2_cap = balf::next_pow2(a.cap);
    const size_t smem = (size_t)a.npow2_cap * 8;
    if (!balf_allow_dynamic_lds<merge_kernel>((int)smem)) return BALF_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    BALF_PROF(balf_prof::kMsMerge, st,
              hipLaunchKernelGGL(merge_kernel, dim3(B), dim3(MERGE_THREADS), smem, st, a));
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
