// The LayerNorm of the training kernels (rcab_train.hip, gmlp_train.hip), ONE forward and ONE backward, at a width C of 256 or
// 128 channels (a template value).  A pixel's C channels lie on C / 4 lanes, four consecutive channels per lane: at C = 256 a wave
// per pixel, at C = 128 two pixels per wave, pixel `sub` = lane >> 5 on its half-wave.  Every sum over the channels is
// (v0 + v1) + (v2 + v3) on the lane and then the xor butterfly C / 8, .. 1 (32..1 at 256, 16..1 inside the half-wave at 128),
// which leaves the same bits on every lane of the pixel.  The variance is taken from the centred values.  The backward
// recomputes xhat = (x - mean) * rstd with the forward's own operations from the saved (mean, rstd), so it is the forward's xhat
// bit for bit, ln_g = 0 or not.  The C channels are a row of a [N,C] matrix or a half of a [N,2C] row: every operand that a
// unit keeps in a wider matrix has an explicit row stride, and a column offset goes into its pointer.  What the backward does
// with a row's input gradient is its template value (LN_DX_*); ln_backward is its launch with the two gradient finishes.
// The float64 partials of dln_g / dln_b of a workgroup's rows [r0, r1): row r0 + k goes to wave (k / P) % 4 and pixel k % P of it,
// P = 256 / C pixels per wave, each (wave, pixel) adds its rows in ascending order; at C = 128 the two pixels of a wave are added
// first (pixel 0 + pixel 1), then the four waves in wave order.  A fixed order that is a function of the sizes alone.
#pragma once
#include "train_gemm.h"

namespace balf {
namespace {

constexpr int kLnFwdPix = 16;               // pixels per workgroup of the LayerNorm forward at C = 256 (four per wave); 32 at 128
constexpr float kLnEps = 1e-5f;

template <int C>
struct LnGeom {
    static_assert(C == 128 || C == 256, "LayerNorm width");
    static constexpr int kLanes = C / 4;            // lanes of a pixel
    static constexpr int kPix = 64 / kLanes;        // pixels per wave
    static constexpr int kFwdPix = kLnFwdPix * kPix;
};

// the sum over a pixel's C channels, four of them on each lane -> every lane of the pixel
template <int C>
__device__ __forceinline__ float chan_sum(gf4 v) {
    float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int o = C / 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// C / 4 lanes per pixel, x[p * xs + c]: n_out [N,C] = xhat * ln_g + ln_b, stat = (mean, rstd)
template <int C>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *x, unsigned xs, const float *ln_g, const float *ln_b, int N,
                                                     float *n_out, float *stat) {
    using G = LnGeom<C>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & (G::kLanes - 1), sub = lane / G::kLanes;
    const gf4 gg = ld4(ln_g + 4 * cl), bb = ld4(ln_b + 4 * cl);
#pragma unroll
    for (int i = 0; i < kLnFwdPix / 4; ++i) {
        const int p0 = blockIdx.x * G::kFwdPix + (4 * i + wave) * G::kPix;   // (uniform in the wave)
        if (p0 >= N) break;
        const bool live = G::kPix == 1 || p0 + sub < N;                     // an odd N leaves the last wave's second pixel empty:
        const int p = live ? p0 + sub : p0;                                 // it recomputes the first and stores nothing
        const gf4 v = ld4(x + row_at(p, xs) + 4 * cl);
        const float mean = chan_sum<C>(v) * (1.0f / C);
        const gf4 d = v - mean;
        const float var = chan_sum<C>(d * d) * (1.0f / C);
        const float rstd = 1.0f / sqrtf(var + kLnEps);
        const gf4 xh = d * rstd;
        gf4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(xh[j], gg[j], bb[j]);
        if (live) {
            st4(n_out + (size_t)p * C + 4 * cl, o);
            if (cl == 0) { stat[2 * (size_t)p] = mean; stat[2 * (size_t)p + 1] = rstd; }
        }
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
    const float *dn, *stat, *ln_g;          // dn [N,C], (mean, rstd) [N,2]
    const float *x, *g, *h;                 // the LayerNorm's input, and what the mode reads
    unsigned xs, gs, hs, os;                // their row strides, and out's
    float *out;
    double *part_g, *part_b;                // [PC][C] each
};

// rows [blockIdx.x * rows, ..) of the pixels, C / 4 lanes per pixel (wave w takes every fourth row, or pair of rows, from w): the
// float64 partials of dln_g = sum dn * xhat and dln_b = sum dn in the order of the file header, and the row's input gradient as
// MODE says
template <int C, int MODE>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdArgs a) {
    using G = LnGeom<C>;
    __shared__ double s_part[2][4][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & (G::kLanes - 1), sub = lane / G::kLanes;
    const int r0 = blockIdx.x * a.rows, r1 = min(a.N, r0 + a.rows);
    const gf4 gg = ld4(a.ln_g + 4 * cl);
    double sg[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p0 = r0 + wave * G::kPix; p0 < r1; p0 += 4 * G::kPix) {
        const bool live = G::kPix == 1 || p0 + sub < r1;        // (the half-wave without a row recomputes the other's, adds and
        const int p = live ? p0 + sub : p0;                     // stores nothing)
        const gf4 dn = ld4(a.dn + (size_t)p * C + 4 * cl), v = ld4(a.x + row_at(p, a.xs) + 4 * cl);
        gf4 hv;                             // (loaded with the row, ahead of the reductions that the tail waits for)
        if constexpr (MODE == LN_DX_GELU || MODE == LN_DX_ADD_GELU) hv = ld4(a.h + row_at(p, a.hs) + 4 * cl);
        const float mean = a.stat[2 * (size_t)p], rstd = a.stat[2 * (size_t)p + 1];
        const gf4 d = v - mean;
        const gf4 xh = d * rstd;
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sg[j] += (double)dn[j] * (double)xh[j];
                sb[j] += (double)dn[j];
            }
        }
        if constexpr (MODE != LN_DX_NONE) {
            const gf4 u = dn * gg;
            const float mu = chan_sum<C>(u) * (1.0f / C), mux = chan_sum<C>(u * xh) * (1.0f / C);
            float *out = a.out + row_at(p, a.os) + 4 * cl;
            gf4 o;
            if constexpr (MODE == LN_DX_ADD) {
                const gf4 gv = ld4(a.g + row_at(p, a.gs) + 4 * cl, a.vec_g);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = gv[j] + rstd * ((u[j] - mu) - xh[j] * mux);
                if (live) st4(out, o, a.vec_out);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = rstd * ((u[j] - mu) - xh[j] * mux);
                if constexpr (MODE == LN_DX_ADD_GELU) o = ld4(a.g + row_at(p, a.gs) + 4 * cl) + o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] *= gelu_grad(hv[j]);
                if (live) st4(out, o);
            }
        }
    }
    if constexpr (G::kPix == 2) {           // the wave's two pixels: pixel 0 + pixel 1 (the same bits on both half-waves)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sg[j] += __shfl_xor(sg[j], 32);
            sb[j] += __shfl_xor(sb[j], 32);
        }
    }
    if (sub == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s_part[0][wave][4 * cl + j] = sg[j];
            s_part[1][wave][4 * cl + j] = sb[j];
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (C < 256 && c >= C) return;
    a.part_g[(size_t)blockIdx.x * C + c] = ((s_part[0][0][c] + s_part[0][1][c]) + s_part[0][2][c]) + s_part[0][3][c];
    a.part_b[(size_t)blockIdx.x * C + c] = ((s_part[1][0][c] + s_part[1][1][c]) + s_part[1][2][c]) + s_part[1][3][c];
}

template <int C>
int ln_forward(const float *x, unsigned xs, const float *ln_g, const float *ln_b, int N, float *n_out, float *stat, hipStream_t st) {
    ln_fwd_kernel<C><<<balf_ceil_div(N, LnGeom<C>::kFwdPix), 256, 0, st>>>(x, xs, ln_g, ln_b, N, n_out, stat);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// the LayerNorm backward over the p.N pixels (a.N and a.rows are set here), then dln_g and dln_b from its partials
template <int C, int MODE>
int ln_backward(LnBwdArgs a, const PixelSlices &p, float *dln_g, float *dln_b, hipStream_t st) {
    a.N = p.N; a.rows = p.col_rows;
    ln_bwd_kernel<C, MODE><<<p.PC, 256, 0, st>>>(a);
    BALF_LAUNCH_CHECK();
    BALF_TRY(finish_cols(a.part_g, C, p.PC, dln_g, st));
    return finish_cols(a.part_b, C, p.PC, dln_b, st);
}

}  // namespace
}  // namespace balf
