// balf_pool_train_forward / balf_pool_train_backward (include/balf_hip.h): the 2 x 2 max-pool that ends a Down stage, in training
// form.  x [B,H,W,C] -> out [B,H/2,W/2,C] and which [B,H/2,W/2,C], a byte per output element: the raster position
// 0..3 of the chosen element in its window ((0,0), (0,1), (1,0), (1,1)).  NHWC float32, C a multiple of 4 up to 256.
// Both kernels: a thread per four consecutive channels of an output pixel, in a grid-stride loop over B * H/2 * W/2 * C/4 such
// quads (at most kPoolMaxWgs workgroups).
//   forward   four 16-byte loads, one 16-byte store, one 4-byte store.  The rule is that of torch's CPU max_pool2d: scan the
//             window in raster order, a value replaces the current one when it is greater or is NaN -- the first maximum wins, of
//             +0 / -0 the first, of several NaN the last.
//   backward  reads g and which alone and writes EVERY element of dx with four 16-byte stores: g at the recorded position, +0.0f
//             at the other three.  No memset, no atomics.
// Nothing is summed, so there is no order to state: two calls give the same bits.
#include "train_gemm.h"

namespace balf {
namespace {

constexpr int kPoolMaxWgs = 2048;           // 256 threads each: eight waves per SIMD of 256 CUs; larger maps take the grid stride
constexpr int kPoolMaxC = 256;

struct PoolGeom {
    int Ho, Wo, cq;                         // the output map; quads per pixel
    size_t quads;                           // B * Ho * Wo * cq
};

// the limits of include/balf_hip.h on (B, H, W, C), H x W the INPUT map
int check_pool_sizes(int B, int H, int W, int C) {
    if (B < 1 || B > kMaxPairs || H < 1 || W < 1) return BALF_ERR_ARG;
    if (C < 4 || C > kPoolMaxC || C % 4) return BALF_ERR_SHAPE;
    if (H % 2 || W % 2) return BALF_ERR_SHAPE;
    if ((long)B * (long)H * (long)W > (long)kTrainMaxN) return BALF_ERR_SHAPE;
    return BALF_OK;
}

PoolGeom pool_geom(int B, int H, int W, int C) {
    PoolGeom g{};
    g.Ho = H / 2; g.Wo = W / 2; g.cq = C / 4;
    g.quads = (size_t)B * g.Ho * g.Wo * g.cq;
    return g;
}

unsigned pool_grid(const PoolGeom &g) {
    const size_t wgs = (g.quads + 255) / 256;
    return (unsigned)(wgs < (size_t)kPoolMaxWgs ? wgs : (size_t)kPoolMaxWgs);
}

// quad q of the output -> the element offset of the window's (0,0) in x / dx; the output's own offset is 4 * q
__device__ __forceinline__ size_t window_at(const PoolGeom &g, size_t q, int C) {
    const size_t pix = q / g.cq;
    const int c = 4 * (int)(q - pix * g.cq);
    const size_t row = pix / g.Wo;          // image * Ho + oy: input row 2 * row of the [B * H, W, C] matrix
    const int ox = (int)(pix - row * g.Wo);
    return ((2 * row) * (size_t)(2 * g.Wo) + 2 * (size_t)ox) * C + c;
}

__global__ __launch_bounds__(256) void pool_fwd_kernel(const float *x, PoolGeom g, int C, float *out, unsigned *which) {
    const size_t step = (size_t)gridDim.x * 256, down = (size_t)(2 * g.Wo) * C;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < g.quads; q += step) {
        const float *w = x + window_at(g, q, C);
        const gf4 v[4] = {ld4(w), ld4(w + C), ld4(w + down), ld4(w + down + C)};
        gf4 best = v[0];
        unsigned at = 0;                    // byte j: the position for channel j
#pragma unroll
        for (int k = 1; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = v[k][j];
                if (e > best[j] || e != e) {
                    best[j] = e;
                    at = (at & ~(0xffu << (8 * j))) | ((unsigned)k << (8 * j));
                }
            }
        st4(out + 4 * q, best);
        which[q] = at;
    }
}

__global__ __launch_bounds__(256) void pool_bwd_kernel(const float *gr, const unsigned *which, PoolGeom g, int C, float *dx) {
    const size_t step = (size_t)gridDim.x * 256, down = (size_t)(2 * g.Wo) * C;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < g.quads; q += step) {
        const gf4 gv = ld4(gr + 4 * q);
        const unsigned at = which[q];
        float *w = dx + window_at(g, q, C);
        gf4 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[k][j] = ((at >> (8 * j)) & 0xffu) == (unsigned)k ? gv[j] : 0.0f;
        st4(w, o[0]);
        st4(w + C, o[1]);
        st4(w + down, o[2]);
        st4(w + down + C, o[3]);
    }
}

}  // namespace

// the unit's two sizes for balf_train_unit_sizes (train_sizes.hip): no workspace, and which as what the backward needs
int pool_train_sizes(int C, int B, int H, int W, size_t *workspace_bytes, size_t *saved_bytes) {
    BALF_TRY(check_pool_sizes(B, H, W, C));
    *workspace_bytes = 0;
    *saved_bytes = 4 * pool_geom(B, H, W, C).quads;
    return BALF_OK;
}

}  // namespace balf

using namespace balf;

extern "C" int balf_pool_train_forward(const float *x_dev, int B, int H, int W, int C, float *out_dev, unsigned char *which_dev,
                                       void *stream) {
    if (!x_dev || !out_dev || !which_dev) return BALF_ERR_ARG;
    if (misaligned(x_dev, 15) || misaligned(out_dev, 15) || misaligned(which_dev, 15)) return BALF_ERR_ARG;
    BALF_TRY(check_pool_sizes(B, H, W, C));
    const PoolGeom g = pool_geom(B, H, W, C);
    pool_fwd_kernel<<<pool_grid(g), 256, 0, static_cast<hipStream_t>(stream)>>>(x_dev, g, C, out_dev,
                                                                                 reinterpret_cast<unsigned *>(which_dev));
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_pool_train_backward(const float *g_dev, const unsigned char *which_dev, int B, int H, int W, int C, float *dx_dev,
                                        void *stream) {
    if (!g_dev || !which_dev || !dx_dev) return BALF_ERR_ARG;
    if (misaligned(g_dev, 15) || misaligned(which_dev, 15) || misaligned(dx_dev, 15)) return BALF_ERR_ARG;
    BALF_TRY(check_pool_sizes(B, H, W, C));
    const PoolGeom g = pool_geom(B, H, W, C);
    pool_bwd_kernel<<<pool_grid(g), 256, 0, static_cast<hipStream_t>(stream)>>>(g_dev, reinterpret_cast<const unsigned *>(which_dev), g,
                                                                                 C, dx_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
