// The LayerNorm pieces of the training kernels (rcab_train.hip, gmlp_train.hip): a pixel's 256 channels on one wave, four
// consecutive channels per lane; every sum over the channels is (v0 + v1) + (v2 + v3) on the lane and then the xor butterfly 32,
// 16, .. 1, which leaves the same bits on every lane.  The variance is taken from the centred values.  The backward recomputes
// xhat = (y - mean) * rstd with the forward's own operations from the saved (mean, rstd), so it is the forward's xhat bit for bit,
// ln_g = 0 or not.
#pragma once
#include "train_gemm.h"

namespace balf {
namespace {

constexpr int kLnFwdPix = 16;               // pixels per workgroup of the LayerNorm forward (four per wave)
constexpr float kLnEps = 1e-5f;

__device__ __forceinline__ gf4 ld4(const float *p) { return *reinterpret_cast<const gf4 *>(p); }
__device__ __forceinline__ void st4(float *p, gf4 v) { *reinterpret_cast<gf4 *>(p) = v; }
// (vec, uniform: the array is 16-byte aligned; else four 4-byte accesses)
__device__ __forceinline__ gf4 ld4(const float *p, bool vec) { return vec ? ld4(p) : gf4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st4(float *p, gf4 v, bool vec) {
    if (vec) { st4(p, v); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = v[j];
}
// the sum over a pixel's 256 channels, four of them on each lane -> every lane
__device__ __forceinline__ float chan_sum(gf4 v) { return wave_sum((v[0] + v[1]) + (v[2] + v[3])); }

// ---- LayerNorm ----------------------------------------------------------------------------------------------------------------
// a wave per pixel: n = xhat * ln_g + ln_b, stat = (mean, rstd)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *y, const float *ln_g, const float *ln_b, int N, float *n_out,
                                                     float *stat) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gf4 gg = ld4(ln_g + 4 * lane), bb = ld4(ln_b + 4 * lane);
#pragma unroll
    for (int i = 0; i < kLnFwdPix / 4; ++i) {
        const int p = blockIdx.x * kLnFwdPix + 4 * i + wave;   // (uniform in the wave)
        if (p >= N) break;
        const size_t at = (size_t)p * kTrainC + 4 * lane;
        const gf4 v = ld4(y + at);
        const float mean = chan_sum(v) * (1.0f / kTrainC);
        const gf4 d = v - mean;
        const float var = chan_sum(d * d) * (1.0f / kTrainC);
        const float rstd = 1.0f / sqrtf(var + kLnEps);
        const gf4 xh = d * rstd;
        gf4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(xh[j], gg[j], bb[j]);
        st4(n_out + at, o);
        if (lane == 0) { stat[2 * (size_t)p] = mean; stat[2 * (size_t)p + 1] = rstd; }
    }
}

struct LnBwdArgs {
    int N, rows;
    bool vec_g, vec_dy;                     // g / dy is 16-byte aligned
    const float *dn, *y, *stat, *ln_g, *g;
    float *dy;
    double *part_g, *part_b;                // [PC][256] each
};

// rows [blockIdx.x * rows, ..) of the pixels, a wave per pixel (wave w takes every fourth row from w): the float64 partials of
// dln_g = sum dn * xhat and dln_b = sum dn, the four waves added in wave order; with WANT_DY
// dy = g + rstd * (u - mean_c u - xhat * mean_c(u * xhat)), u = dn * ln_g
template <bool WANT_DY>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdArgs a) {
    __shared__ double s_part[2][4][kTrainC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
    const gf4 gg = ld4(a.ln_g + 4 * lane);
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = r0 + wave; p < r1; p += 4) {
        const size_t at = (size_t)p * kTrainC + 4 * lane;
        const gf4 dn = ld4(a.dn + at), v = ld4(a.y + at);
        const float mean = a.stat[2 * (size_t)p], rstd = a.stat[2 * (size_t)p + 1];
        const gf4 d = v - mean;
        const gf4 xh = d * rstd;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sg[j] += (double)dn[j] * (double)xh[j];
            sb[j] += (double)dn[j];
        }
        if constexpr (WANT_DY) {
            const gf4 u = dn * gg;
            const float mu = chan_sum(u) * (1.0f / kTrainC), mux = chan_sum(u * xh) * (1.0f / kTrainC);
            const gf4 gv = ld4(a.g + at, a.vec_g);
            gf4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = gv[j] + rstd * ((u[j] - mu) - xh[j] * mux);
            st4(a.dy + at, o, a.vec_dy);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_part[0][wave][4 * lane + j] = sg[j];
        s_part[1][wave][4 * lane + j] = sb[j];
    }
    __syncthreads();
    const int c = threadIdx.x;
    a.part_g[(size_t)blockIdx.x * kTrainC + c] = ((s_part[0][0][c] + s_part[0][1][c]) + s_part[0][2][c]) + s_part[0][3][c];
    a.part_b[(size_t)blockIdx.x * kTrainC + c] = ((s_part[1][0][c] + s_part[1][1][c]) + s_part[1][2][c]) + s_part[1][3][c];
}

}  // namespace
}  // namespace balf
