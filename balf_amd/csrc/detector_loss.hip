// balf_detector_loss (include/balf_hip.h): the reference's detector_loss (balf/loss/loss_function.py:7-26) for the 65-channel
// head and its gradient with respect to the logits, one pass over the logits.
//
// One lane owns one cell; consecutive lanes take consecutive cells of the flattened [Hc*Wc] plane, so each of the 65 channel
// loads (and gradient stores) of a wave is one contiguous 256-byte line, and the 8 x 8 pixels of a cell are 2 x float4 per
// row, contiguous across the lanes of a row of cells.  Four launches:
//   1. loss_mask_kernel    mask -> vm per cell (workspace) and the float64 partial sums of fl32(vm + 1e-6f), one per workgroup
//   2. loss_sum_kernel     den_b: a wave per image sums the image's partials in fixed order
//   3. loss_cells_kernel   key points + noise -> label; 65 logits into registers -> log-sum-exp, ce, the gradient (which needs
//                          den_b, hence launches 1-2 first); float64 partial sums of ce * vm, one per workgroup
//   4. loss_finish_kernel  num_b / den_b per image (a wave per image), then their mean in index order
// Bytes: the mask, the key-point map, the noise and the logits are read once, vm (4 bytes per cell) is written and read once.
// Every sum is float64 in an order fixed by (Hc, Wc): lanes of a wave by xor butterfly, waves of a workgroup in order
// (block_sum), workgroups of an image strided over the lanes of one wave and then the same butterfly.
#include "block_ops.h"

namespace balf {
namespace {

constexpr int kLossThreads = 256;           // lanes = cells per workgroup of launches 1 and 3
constexpr int kLossChannels = 65;           // 8 x 8 positions and the dustbin
constexpr int kLossMaxCells = 1 << 24;      // cells per image: the workgroup index of an image stays a grid x dimension
constexpr int kSumThreads = 256;            // launch 2: four images per workgroup
constexpr int kFinishThreads = 1024;        // launch 4: ONE workgroup, sixteen images at a time

struct LossArgs {
    const float *logits, *kp, *mask, *noise;
    int B, Hc, Wc, n, nblk;
    bool vec;                               // kp and mask are 16-byte aligned: float4 loads
    float *loss, *per_image, *dlogits;
    int32_t *labels;
    float *vm;                              // [B, n]       cell masks (only with a mask)
    double *den_part, *num_part;            // [B, nblk]
    double *den, *ratio;                    // [B]
};

// the 8 floats of row dy of a cell's 8 x 8 pixels
__device__ __forceinline__ void load_row8(const float *p, bool vec, float (&v)[8]) {
    if (vec) {
        const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i];
    }
}

// offset of pixel (8y, 8x) of cell `cell` of image b in a [B,1,8Hc,8Wc] map
__device__ __forceinline__ size_t cell_pixel0(const LossArgs &a, int b, int cell) {
    const int y = cell / a.Wc, x = cell - y * a.Wc;
    return (size_t)b * 64u * (size_t)a.n + (size_t)(8 * y) * (size_t)(8 * a.Wc) + (size_t)(8 * x);
}

// sum of an image's nblk per-workgroup partials, to every lane of the wave
__device__ __forceinline__ double wave_sum_partials(const double *part, int nblk) {
    double s = 0.0;
    for (int i = threadIdx.x & 63; i < nblk; i += 64) s += part[i];
    return wave_sum(s);
}

__global__ __launch_bounds__(kLossThreads) void loss_mask_kernel(LossArgs a) {
    __shared__ double s_red[kLossThreads / 64];
    const int b = blockIdx.y, cell = blockIdx.x * kLossThreads + threadIdx.x;
    double d = 0.0;
    if (cell < a.n) {
        float vm = 1.0f;
        if (a.mask) {
            const float *p = a.mask + cell_pixel0(a, b, cell);
#pragma unroll
            for (int dy = 0; dy < 8; ++dy) {
                float v[8];
                load_row8(p + (size_t)dy * (size_t)(8 * a.Wc), a.vec, v);
#pragma unroll
                for (int dx = 0; dx < 8; ++dx) vm *= v[dx];
            }
            a.vm[(size_t)b * a.n + cell] = vm;
        }
        d = (double)(vm + 1e-6f);
    }
    d = block_sum<kLossThreads>(d, s_red);
    if (threadIdx.x == 0) a.den_part[(size_t)b * a.nblk + blockIdx.x] = d;
}

__global__ __launch_bounds__(kSumThreads) void loss_sum_kernel(LossArgs a) {
    const int b = blockIdx.x * (kSumThreads / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const double s = wave_sum_partials(a.den_part + (size_t)b * a.nblk, a.nblk);
    if ((threadIdx.x & 63) == 0) a.den[b] = s;
}

__global__ __launch_bounds__(kLossThreads) void loss_cells_kernel(LossArgs a) {
    __shared__ double s_red[kLossThreads / 64];
    const int b = blockIdx.y, cell = blockIdx.x * kLossThreads + threadIdx.x;
    double num = 0.0;
    if (cell < a.n) {
        const size_t n = (size_t)a.n, at = (size_t)b * kLossChannels * n + (size_t)cell;      // channel 0 of this cell
        // the 65 logits first: the longest loads of the lane are in flight while the label is worked out
        float z[kLossChannels];
#pragma unroll
        for (int c = 0; c < kLossChannels; ++c) z[c] = a.logits[at + (size_t)c * n];
        // label: first index of the maximum of 2 * kp + noise over the 64 positions and of 1 + noise over the dustbin
        const float *kp = a.kp + cell_pixel0(a, b, cell);
        const float *nz = a.noise ? a.noise + at : nullptr;
        float best = 0.0f;
        int label = 0;
#pragma unroll
        for (int dy = 0; dy < 8; ++dy) {
            float v[8];
            load_row8(kp + (size_t)dy * (size_t)(8 * a.Wc), a.vec, v);
#pragma unroll
            for (int dx = 0; dx < 8; ++dx) {
                const int c = dy * 8 + dx;
                float t = 2.0f * v[dx];                                     // exact
                if (nz) t = t + nz[(size_t)c * n];
                if (c == 0 || t > best) { best = t; label = c; }
            }
        }
        {
            const float t = nz ? 1.0f + nz[(size_t)64 * n] : 1.0f;
            if (t > best) label = 64;
        }
        const float vm = a.mask ? a.vm[(size_t)b * n + cell] : 1.0f;
        // log-sum-exp with the maximum taken out; z[c] becomes exp(z[c] - max)
        float m = z[0], zl = z[0];
#pragma unroll
        for (int c = 1; c < kLossChannels; ++c) {
            m = fmaxf(m, z[c]);
            zl = c == label ? z[c] : zl;
        }
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < kLossChannels; ++c) {
            z[c] = expf(z[c] - m);
            s += (double)z[c];
        }
        const double ce = ((double)m - (double)zl) + log(s);
        num = ce * (double)vm;
        if (a.labels) a.labels[(size_t)b * n + cell] = label;
        if (a.dlogits) {
            const double inv_s = 1.0 / s, scale = (double)vm / (a.den[b] * (double)a.B);
#pragma unroll
            for (int c = 0; c < kLossChannels; ++c)
                a.dlogits[at + (size_t)c * n] = (float)(((double)z[c] * inv_s - (c == label ? 1.0 : 0.0)) * scale);
        }
    }
    num = block_sum<kLossThreads>(num, s_red);
    if (threadIdx.x == 0) a.num_part[(size_t)b * a.nblk + blockIdx.x] = num;
}

__global__ __launch_bounds__(kFinishThreads) void loss_finish_kernel(LossArgs a) {
    for (int b = threadIdx.x >> 6; b < a.B; b += kFinishThreads / 64) {
        const double r = wave_sum_partials(a.num_part + (size_t)b * a.nblk, a.nblk) / a.den[b];
        if ((threadIdx.x & 63) == 0) {
            a.ratio[b] = r;
            if (a.per_image) a.per_image[b] = (float)r;
        }
    }
    __syncthreads();                        // the ratios were written by this workgroup: visible to it after the barrier
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < a.B; ++b) s += a.ratio[b];
        a.loss[0] = (float)(s / (double)a.B);
    }
}

bool loss_sizes_ok(int B, int Hc, int Wc) {
    return B >= 1 && B <= kMaxPairs && Hc >= 1 && Wc >= 1 && (long)Hc * (long)Wc <= (long)kLossMaxCells;
}

// the workspace layout; returns its size
size_t loss_layout(LossArgs &a, char *base) {
    WorkspaceCursor ws{base, 0};
    const size_t cells = (size_t)a.B * (size_t)a.n, parts = (size_t)a.B * (size_t)a.nblk;
    a.vm = ws.take<float>(cells * sizeof(float));
    a.den_part = ws.take<double>(parts * sizeof(double));
    a.num_part = ws.take<double>(parts * sizeof(double));
    a.den = ws.take<double>((size_t)a.B * sizeof(double));
    a.ratio = ws.take<double>((size_t)a.B * sizeof(double));
    return ws.used;
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_detector_loss_workspace_bytes(int B, int Hc, int Wc) {
    if (!loss_sizes_ok(B, Hc, Wc)) return 0;
    LossArgs a{};
    a.B = B;
    a.n = Hc * Wc;
    a.nblk = balf_ceil_div(a.n, kLossThreads);
    return loss_layout(a, nullptr);
}

extern "C" int balf_detector_loss(const float *logits_dev, const float *keypoint_map_dev, const float *valid_mask_dev,
                                  const float *noise_dev, int B, int Hc, int Wc, float *loss_dev, float *per_image_dev,
                                  int32_t *labels_dev, float *dlogits_dev, void *workspace_dev, size_t workspace_bytes,
                                  void *stream) {
    if (!logits_dev || !keypoint_map_dev || !loss_dev || !workspace_dev) return BALF_ERR_ARG;
    if ((uintptr_t)workspace_dev & 7u) return BALF_ERR_ARG;                 // float64 partial sums live in it
    if (B < 1 || B > kMaxPairs || Hc < 1 || Wc < 1) return BALF_ERR_ARG;
    if ((long)Hc * (long)Wc > (long)kLossMaxCells) return BALF_ERR_SHAPE;
    if (workspace_bytes < balf_detector_loss_workspace_bytes(B, Hc, Wc)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossArgs a{};
    a.logits = logits_dev;
    a.kp = keypoint_map_dev;
    a.mask = valid_mask_dev;
    a.noise = noise_dev;
    a.B = B;
    a.Hc = Hc;
    a.Wc = Wc;
    a.n = Hc * Wc;
    a.nblk = balf_ceil_div(a.n, kLossThreads);
    // rows of 8 * Wc floats and cells of 8: every row of every cell is 16-byte aligned when the maps are
    a.vec = (((uintptr_t)keypoint_map_dev | (uintptr_t)valid_mask_dev) & 15u) == 0;
    a.loss = loss_dev;
    a.per_image = per_image_dev;
    a.labels = labels_dev;
    a.dlogits = dlogits_dev;
    loss_layout(a, static_cast<char *>(workspace_dev));
    const dim3 cells_grid(a.nblk, B);
    loss_mask_kernel<<<cells_grid, kLossThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    loss_sum_kernel<<<balf_ceil_div(B, kSumThreads / 64), kSumThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    loss_cells_kernel<<<cells_grid, kLossThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    loss_finish_kernel<<<1, kFinishThreads, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
