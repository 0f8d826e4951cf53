// The LayerNorm of the training kernels (rcab_train.hip, gmlp_train.hip), ONE forward and ONE backward: a pixel's 256 channels on
// one wave, four consecutive channels per lane; every sum over the channels is (v0 + v1) + (v2 + v3) on the lane and then the xor
// butterfly 32, 16, .. 1, which leaves the same bits on every lane.  The variance is taken from the centred values.  The backward
// recomputes xhat = (x - mean) * rstd with the forward's own operations from the saved (mean, rstd), so it is the forward's xhat
// bit for bit, ln_g = 0 or not.  The 256 channels are a row of a [N,256] matrix or a half of a [N,512] row: every operand that a
// unit keeps in a wider matrix has an explicit row stride, and a column offset goes into its pointer.  What the backward does
// with a row's input gradient is its template value (LN_DX_*); ln_backward is its launch with the two gradient finishes.
#pragma once
#include "train_gemm.h"

namespace balf {
namespace {

constexpr int kLnFwdPix = 16;               // pixels per workgroup of the LayerNorm forward (four per wave)
constexpr float kLnEps = 1e-5f;

// the sum over a pixel's 256 channels, four of them on each lane -> every lane
__device__ __forceinline__ float chan_sum(gf4 v) { return wave_sum((v[0] + v[1]) + (v[2] + v[3])); }

// a wave per pixel, x[p * xs + c]: n_out [N,256] = xhat * ln_g + ln_b, stat = (mean, rstd)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *x, unsigned xs, const float *ln_g, const float *ln_b, int N,
                                                     float *n_out, float *stat) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gf4 gg = ld4(ln_g + 4 * lane), bb = ld4(ln_b + 4 * lane);
#pragma unroll
    for (int i = 0; i < kLnFwdPix / 4; ++i) {
        const int p = blockIdx.x * kLnFwdPix + 4 * i + wave;   // (uniform in the wave)
        if (p >= N) break;
        const gf4 v = ld4(x + row_at(p, xs) + 4 * lane);
        const float mean = chan_sum(v) * (1.0f / kTrainC);
        const gf4 d = v - mean;
        const float var = chan_sum(d * d) * (1.0f / kTrainC);
        const float rstd = 1.0f / sqrtf(var + kLnEps);
        const gf4 xh = d * rstd;
        gf4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(xh[j], gg[j], bb[j]);
        st4(n_out + (size_t)p * kTrainC + 4 * lane, o);
        if (lane == 0) { stat[2 * (size_t)p] = mean; stat[2 * (size_t)p + 1] = rstd; }
    }
}

// What becomes of a row's input gradient L = rstd * (u - mean_c u - xhat * mean_c(u * xhat)), u = dn * ln_g:
//   LN_DX_NONE      nothing: not computed, not stored
//   LN_DX_ADD       out = g + L; g and out may start 4 bytes off a 16-byte boundary (vec_g, vec_out)
//   LN_DX_GELU      out = L * gelu'(h)
//   LN_DX_ADD_GELU  out = (g + L) * gelu'(h)
// g: the gradient that reaches the LayerNorm's input past it (a shortcut); h: the pre-activation of the GELU that made that input,
// so that dH = dG * gelu'(H) costs no pass of its own.
enum { LN_DX_NONE = 0, LN_DX_ADD = 1, LN_DX_GELU = 2, LN_DX_ADD_GELU = 3 };

struct LnBwdArgs {
    int N, rows;
    bool vec_g, vec_out;                    // LN_DX_ADD: g / out is 16-byte aligned
    const float *dn, *stat, *ln_g;          // dn [N,256], (mean, rstd) [N,2]
    const float *x, *g, *h;                 // the LayerNorm's input, and what the mode reads
    unsigned xs, gs, hs, os;                // their row strides, and out's
    float *out;
    double *part_g, *part_b;                // [PC][256] each
};

// rows [blockIdx.x * rows, ..) of the pixels, a wave per pixel (wave w takes every fourth row from w): the float64 partials of
// dln_g = sum dn * xhat and dln_b = sum dn, the four waves added in wave order, and the row's input gradient as MODE says
template <int MODE>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdArgs a) {
    __shared__ double s_part[2][4][kTrainC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
    const gf4 gg = ld4(a.ln_g + 4 * lane);
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = r0 + wave; p < r1; p += 4) {
        const gf4 dn = ld4(a.dn + (size_t)p * kTrainC + 4 * lane), v = ld4(a.x + row_at(p, a.xs) + 4 * lane);
        gf4 hv;                             // (loaded with the row, ahead of the reductions that the tail waits for)
        if constexpr (MODE == LN_DX_GELU || MODE == LN_DX_ADD_GELU) hv = ld4(a.h + row_at(p, a.hs) + 4 * lane);
        const float mean = a.stat[2 * (size_t)p], rstd = a.stat[2 * (size_t)p + 1];
        const gf4 d = v - mean;
        const gf4 xh = d * rstd;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sg[j] += (double)dn[j] * (double)xh[j];
            sb[j] += (double)dn[j];
        }
        if constexpr (MODE != LN_DX_NONE) {
            const gf4 u = dn * gg;
            const float mu = chan_sum(u) * (1.0f / kTrainC), mux = chan_sum(u * xh) * (1.0f / kTrainC);
            float *out = a.out + row_at(p, a.os) + 4 * lane;
            gf4 o;
            if constexpr (MODE == LN_DX_ADD) {
                const gf4 gv = ld4(a.g + row_at(p, a.gs) + 4 * lane, a.vec_g);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = gv[j] + rstd * ((u[j] - mu) - xh[j] * mux);
                st4(out, o, a.vec_out);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = rstd * ((u[j] - mu) - xh[j] * mux);
                if constexpr (MODE == LN_DX_ADD_GELU) o = ld4(a.g + row_at(p, a.gs) + 4 * lane) + o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] *= gelu_grad(hv[j]);
                st4(out, o);
            }
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

// the LayerNorm backward over the p.N pixels (a.N and a.rows are set here), then dln_g and dln_b from its partials
template <int MODE>
int ln_backward(LnBwdArgs a, const PixelSlices &p, float *dln_g, float *dln_b, hipStream_t st) {
    a.N = p.N; a.rows = p.col_rows;
    ln_bwd_kernel<MODE><<<p.PC, 256, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    BALF_TRY(finish_cols(a.part_g, kTrainC, p.PC, dln_g, st));
    return finish_cols(a.part_b, kTrainC, p.PC, dln_b, st);
}

}  // namespace
}  // namespace balf
