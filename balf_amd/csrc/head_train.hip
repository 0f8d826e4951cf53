// balf_head_train_forward / balf_head_train_backward (include/balf_hip.h): the trainable tail of the detector,
//   x2 -> down4.conv2 (Linear 256 -> 256) -> ReLU -> detector_head.dense (Linear 256 -> 65) -> BatchNorm2d with BATCH statistics,
// and its backward from dlogits to the six parameter gradients and dx2.  N = B * Hc * Wc pixels.
//
// Three kinds of kernels:
//   * gemm_kernel (train_gemm.h, shared with the other training units, as are the argument rule check_sizes and the launch
//     helpers): ONE LDS-tiled GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains, k ascending) for all six products.  A
//     workgroup of four waves owns a 64 x 64 tile of C[m][n] = sum_k A(m,k) * B(k,n), a wave a 32 x 32 quarter (2 x 2 MFMA tiles);
//     K goes through LDS in steps of 16 with the next step's operands fetched into registers before the MFMAs of this one.  The
//     operands are addressed by (row stride, k stride), so the same kernel reads x2 [N,256], the weights in PyTorch layout and the
//     channel-major z / dz [65,N]; whatever lies outside M, Nn or the K range is never loaded and enters the tile as 0, and a 16-row
//     MFMA tile wholly outside is skipped: the 65-wide side is padded here, in the kernel, and no pad value is ever stored.
//     The weight gradients sum over the pixels: their K range is cut into S slices (rows_per_slice(N)), slice s writes slab s of
//     the workspace, and slab_sum_kernel adds the S slabs in float64 in slice order.
//   * row kernels over the channel-major [65,N] arrays, a pixel on the lane: the batch statistics (float64 sums of z and z * z),
//     dbeta / dgamma (float64), dz and its sum, each as per-workgroup partials [65][P] that a wave per channel adds in one fixed
//     order (lanes strided over the partials, then the butterfly).
//   * db2, the column sums of the pixel-major dh [N,256]: bias_grad of train_gemm.h (col_sum_kernel, then partial_sum_kernel).
// No floating-point atomics anywhere; every order is a function of N alone.
// saved: a = relu(h) [N,256] (h > 0 exactly where a > 0), z channel-major [65,N], and mean / 1/sqrt(var + eps) as float64.
#include "train_gemm.h"

namespace balf {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kC = 256;                     // channels of x2, of down4.conv2 and of the head's input
constexpr int kZ = 65;                      // head channels
constexpr int kRowThreads = 256;
constexpr int kRowChunk = 4 * kRowThreads;  // pixels per workgroup of the row kernels

struct Layout {
    int P;                                  // row-kernel partials per channel
    PixelSlices px;
    // saved
    float *a, *zT;
    double *stat;                           // [2][65]: mean, 1 / sqrt(var + eps)
    // workspace
    double *part;                           // [2][65][P]
    double *dbn;                            // [2][65]: dbeta, dgamma
    double *b2_part;                        // [PC][256]
    float *dzT, *dh, *slab_wd, *slab_w2;
};

Layout make_layout(int N, char *saved, char *work, size_t *saved_bytes, size_t *work_bytes) {
    Layout l{};
    l.P = balf_ceil_div(N, kRowChunk);
    l.px = pixel_slices(N);
    WorkspaceCursor sv{saved, 0};
    l.a = sv.take<float>((size_t)N * kC * sizeof(float));
    l.zT = sv.take<float>((size_t)N * kZ * sizeof(float));
    l.stat = sv.take<double>(2 * kZ * sizeof(double));
    if (saved_bytes) *saved_bytes = sv.used;
    WorkspaceCursor ws{work, 0};
    l.part = ws.take<double>((size_t)2 * kZ * l.P * sizeof(double));
    l.dbn = ws.take<double>(2 * kZ * sizeof(double));
    l.b2_part = ws.take<double>((size_t)l.px.PC * kC * sizeof(double));
    l.dzT = ws.take<float>((size_t)N * kZ * sizeof(float));
    l.dh = ws.take<float>((size_t)N * kC * sizeof(float));
    l.slab_wd = ws.take<float>((size_t)l.px.S * kZ * kC * sizeof(float));
    l.slab_w2 = ws.take<float>((size_t)l.px.S * kC * kC * sizeof(float));
    if (work_bytes) *work_bytes = ws.used;
    return l;
}

// ---- the row kernels ----------------------------------------------------------------------------------------------------------
struct RowArgs {
    int N, hw, P;
    const float *zT, *g, *gamma;            // g = dlogits [B,65,Hc,Wc]
    const double *stat, *dbn;
    float *dzT;
    double *part;                           // [2][65][P]
};

__device__ __forceinline__ float xhat_of(float z, double mean, double rstd) { return (float)(((double)z - mean) * rstd); }

enum { ROW_STATS = 0, ROW_DBN = 1, ROW_DZ = 2 };

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void row_kernel(RowArgs a) {
    __shared__ double s_red[kRowThreads / 64];
    const int c = blockIdx.y;
    const size_t row = (size_t)c * (size_t)a.N;
    double mean = 0.0, rstd = 0.0, k_g = 0.0, k_b = 0.0, k_x = 0.0;
    if (MODE != ROW_STATS) { mean = a.stat[c]; rstd = a.stat[kZ + c]; }
    if (MODE == ROW_DZ) {
        k_g = (double)a.gamma[c] * rstd;
        k_b = a.dbn[c] / (double)a.N;
        k_x = a.dbn[kZ + c] / (double)a.N;
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const int p = blockIdx.x * kRowChunk + i * kRowThreads + (int)threadIdx.x;
        if (p >= a.N) continue;
        const float z = a.zT[row + p];
        if (MODE == ROW_STATS) {
            s0 += (double)z;
            s1 += (double)z * (double)z;
        } else {
            const int b = p / a.hw, o = p - b * a.hw;
            // xhat stays float64 here: with few pixels g - dbeta / N - xhat dgamma / N cancels almost completely (N = 2: to eps / var),
            // and a float32 rounding of xhat would be all that is left of it
            const double gv = (double)a.g[((size_t)b * kZ + c) * (size_t)a.hw + o], xh = ((double)z - mean) * rstd;
            if (MODE == ROW_DBN) {
                s0 += gv;
                s1 += gv * xh;
            } else {
                const float dz = (float)(k_g * (gv - k_b - xh * k_x));
                a.dzT[row + p] = dz;
                s0 += (double)dz;
            }
        }
    }
    s0 = block_sum<kRowThreads>(s0, s_red);
    if (MODE != ROW_DZ) s1 = block_sum<kRowThreads>(s1, s_red);
    if (threadIdx.x == 0) {
        a.part[(size_t)c * a.P + blockIdx.x] = s0;
        if (MODE != ROW_DZ) a.part[((size_t)kZ + c) * a.P + blockIdx.x] = s1;
    }
}

struct StatArgs {
    int N, P, use_stats;
    const double *part;
    const float *stats_in;                  // [2][65] mean, var (use_stats)
    double eps, momentum;
    double *stat;
    float *running_mean, *running_var;
};

// one wave per channel: mean, biased variance -> saved statistics; the running statistics if asked for
__global__ __launch_bounds__(64) void stat_finish_kernel(StatArgs a) {
    const int c = blockIdx.x;
    double mean, var;
    if (a.use_stats) {
        mean = (double)a.stats_in[c];
        var = (double)a.stats_in[kZ + c];
    } else {
        const double s1 = wave_sum_strided(a.part + (size_t)c * a.P, a.P, 1), s2 = wave_sum_strided(a.part + ((size_t)kZ + c) * a.P, a.P, 1);
        mean = s1 / (double)a.N;
        var = fmax(s2 / (double)a.N - mean * mean, 0.0);
    }
    if (threadIdx.x != 0) return;
    a.stat[c] = mean;
    a.stat[kZ + c] = 1.0 / sqrt(var + a.eps);
    if (a.use_stats) return;
    if (a.running_mean) a.running_mean[c] = (float)((1.0 - a.momentum) * (double)a.running_mean[c] + a.momentum * mean);
    if (a.running_var)
        a.running_var[c] = (float)((1.0 - a.momentum) * (double)a.running_var[c] + a.momentum * (var * (double)a.N / (double)(a.N - 1)));
}

struct NormArgs {
    int N, hw, Hc, Wc;
    bool vec;                               // prob is 16-byte aligned: float4 stores
    const float *zT, *gamma, *beta;
    const double *stat;
    float *logits, *prob;
};

// a pixel per lane: logits (NCHW) = gamma * xhat + beta; with PROB the softmax over the 65 logits, dustbin dropped, pixel-shuffled
template <bool PROB>
__global__ __launch_bounds__(256) void normalize_kernel(NormArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.N) return;
    const int b = p / a.hw, o = p - b * a.hw;
    float l[PROB ? kZ : 1];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < kZ; ++c) {
        const float xh = xhat_of(a.zT[(size_t)c * a.N + p], a.stat[c], a.stat[kZ + c]);
        const float v = fmaf(a.gamma[c], xh, a.beta[c]);
        a.logits[((size_t)b * kZ + c) * (size_t)a.hw + o] = v;
        if constexpr (PROB) { l[c] = v; mx = fmaxf(mx, v); }
    }
    if constexpr (PROB) {
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < kZ; ++c) {
            l[c] = expf(l[c] - mx);
            sum += l[c];
        }
        const float inv = 1.0f / sum;
        const int y = o / a.Wc, x = o - y * a.Wc;
        float *dst = a.prob + ((size_t)b * 8 * a.Hc + 8 * y) * (size_t)(8 * a.Wc) + 8 * x;
#pragma unroll
        for (int dy = 0; dy < 8; ++dy) {
            float *d = dst + (size_t)dy * (size_t)(8 * a.Wc);
            if (a.vec) {
                reinterpret_cast<f4 *>(d)[0] = f4{l[8 * dy] * inv, l[8 * dy + 1] * inv, l[8 * dy + 2] * inv, l[8 * dy + 3] * inv};
                reinterpret_cast<f4 *>(d)[1] = f4{l[8 * dy + 4] * inv, l[8 * dy + 5] * inv, l[8 * dy + 6] * inv, l[8 * dy + 7] * inv};
            } else {
#pragma unroll
                for (int dx = 0; dx < 8; ++dx) d[dx] = l[8 * dy + dx] * inv;
            }
        }
    }
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_head_train_workspace_bytes(long N) {
    if (N < 2 || N > (long)kTrainMaxN) return 0;
    size_t bytes = 0;
    make_layout((int)N, nullptr, nullptr, nullptr, &bytes);
    return bytes;
}

extern "C" size_t balf_head_train_saved_bytes(long N) {
    if (N < 2 || N > (long)kTrainMaxN) return 0;
    size_t bytes = 0;
    make_layout((int)N, nullptr, nullptr, &bytes, nullptr);
    return bytes;
}

extern "C" int balf_head_train_forward(const float *x2_dev, const float *w2_dev, const float *b2_dev, const float *wd_dev,
                                       const float *bd_dev, const float *gamma_dev, const float *beta_dev, int B, int Hc, int Wc,
                                       double eps, int use_stats, const float *stats_in_dev, float *logits_dev, float *prob_dev,
                                       float *running_mean_dev, float *running_var_dev, double momentum, void *saved_dev,
                                       void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!x2_dev || !w2_dev || !b2_dev || !wd_dev || !bd_dev || !gamma_dev || !beta_dev || !logits_dev || !saved_dev || !workspace_dev)
        return BALF_ERR_ARG;
    if (use_stats && !stats_in_dev) return BALF_ERR_ARG;
    if (misaligned(saved_dev, 7) || misaligned(workspace_dev, 7)) return BALF_ERR_ARG;      // float64 statistics and partial sums
    if (!(eps >= 0.0)) return BALF_ERR_ARG;
    const int rc = check_sizes(B, Hc, Wc);
    if (rc != BALF_OK) return rc;
    const int N = B * Hc * Wc;
    if (workspace_bytes < balf_head_train_workspace_bytes(N)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout l = make_layout(N, static_cast<char *>(saved_dev), static_cast<char *>(workspace_dev), nullptr, nullptr);

    // a[pixel][out] = relu(sum_k x2[pixel][k] * W2[out][k] + b2[out])
    BALF_TRY((pixel_gemm<EPI_BIAS_N_RELU, false>(x2_dev, kC, kC, w2_dev, kC, N, l.a, kC, b2_dev, nullptr, st)));
    // zT[c][pixel] = sum_k Wd[c][k] * a[pixel][k] + bd[c]
    GemmArgs g{};
    g.A = wd_dev; g.a_sm = kC; g.a_sk = 1;
    g.B = l.a; g.b_sn = kC; g.b_sk = 1;
    g.M = kZ; g.Nn = N; g.K = kC; g.k_rows = kC;
    g.C = l.zT; g.c_sm = (size_t)N; g.bias = bd_dev;
    launch_gemm<true, true, true, EPI_BIAS_M>(g, st);
    BALF_LAUNCH_CHECK();

    if (!use_stats) {
        RowArgs r{};
        r.N = N; r.hw = Hc * Wc; r.P = l.P; r.zT = l.zT; r.part = l.part;
        row_kernel<ROW_STATS><<<dim3(l.P, kZ), kRowThreads, 0, st>>>(r);
        BALF_LAUNCH_CHECK();
    }
    StatArgs s{};
    s.N = N; s.P = l.P; s.use_stats = use_stats ? 1 : 0; s.part = l.part; s.stats_in = stats_in_dev;
    s.eps = eps; s.momentum = momentum; s.stat = l.stat;
    s.running_mean = running_mean_dev; s.running_var = running_var_dev;
    stat_finish_kernel<<<kZ, 64, 0, st>>>(s);
    BALF_LAUNCH_CHECK();

    NormArgs n{};
    n.N = N; n.hw = Hc * Wc; n.Hc = Hc; n.Wc = Wc;
    n.vec = ((uintptr_t)prob_dev & 15u) == 0;
    n.zT = l.zT; n.gamma = gamma_dev; n.beta = beta_dev; n.stat = l.stat;
    n.logits = logits_dev; n.prob = prob_dev;
    if (prob_dev) normalize_kernel<true><<<balf_ceil_div(N, 256), 256, 0, st>>>(n);
    else normalize_kernel<false><<<balf_ceil_div(N, 256), 256, 0, st>>>(n);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_head_train_backward(const float *dlogits_dev, const float *x2_dev, const float *w2_dev, const float *wd_dev,
                                        const float *gamma_dev, const void *saved_dev, int B, int Hc, int Wc, float *dw2_dev,
                                        float *db2_dev, float *dwd_dev, float *dbd_dev, float *dgamma_dev, float *dbeta_dev,
                                        float *dx2_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!dlogits_dev || !x2_dev || !w2_dev || !wd_dev || !gamma_dev || !saved_dev || !dw2_dev || !db2_dev || !dwd_dev || !dbd_dev ||
        !dgamma_dev || !dbeta_dev || !workspace_dev)
        return BALF_ERR_ARG;
    if (misaligned(saved_dev, 7) || misaligned(workspace_dev, 7)) return BALF_ERR_ARG;
    const int rc = check_sizes(B, Hc, Wc);
    if (rc != BALF_OK) return rc;
    const int N = B * Hc * Wc;
    if (workspace_bytes < balf_head_train_workspace_bytes(N)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout l = make_layout(N, static_cast<char *>(const_cast<void *>(saved_dev)), static_cast<char *>(workspace_dev), nullptr, nullptr);

    // BatchNorm: dbeta, dgamma, then dz (channel-major) and dbd = sum dz
    RowArgs r{};
    r.N = N; r.hw = Hc * Wc; r.P = l.P; r.zT = l.zT; r.g = dlogits_dev; r.gamma = gamma_dev;
    r.stat = l.stat; r.dbn = l.dbn; r.dzT = l.dzT; r.part = l.part;
    row_kernel<ROW_DBN><<<dim3(l.P, kZ), kRowThreads, 0, st>>>(r);
    BALF_LAUNCH_CHECK();
    partial_sum_kernel<<<balf_ceil_div(kZ, 4), 256, 0, st>>>(l.part, kZ, l.P, (size_t)l.P, 1, dbeta_dev, l.dbn);
    BALF_LAUNCH_CHECK();
    partial_sum_kernel<<<balf_ceil_div(kZ, 4), 256, 0, st>>>(l.part + (size_t)kZ * l.P, kZ, l.P, (size_t)l.P, 1, dgamma_dev, l.dbn + kZ);
    BALF_LAUNCH_CHECK();
    row_kernel<ROW_DZ><<<dim3(l.P, kZ), kRowThreads, 0, st>>>(r);
    BALF_LAUNCH_CHECK();
    partial_sum_kernel<<<balf_ceil_div(kZ, 4), 256, 0, st>>>(l.part, kZ, l.P, (size_t)l.P, 1, dbd_dev, nullptr);
    BALF_LAUNCH_CHECK();

    // dWd[c][k] = sum_pixel dzT[c][pixel] * a[pixel][k], in S slices of the pixels
    GemmArgs g{};
    g.A = l.dzT; g.a_sm = (size_t)N; g.a_sk = 1;
    g.B = l.a; g.b_sn = 1; g.b_sk = kC;
    g.M = kZ; g.Nn = kC; g.K = N; g.k_rows = l.px.rows;
    g.C = l.slab_wd; g.c_sm = kC; g.c_sz = (size_t)kZ * kC;
    launch_gemm<true, false, false, EPI_STORE>(g, st);
    BALF_LAUNCH_CHECK();
    slab_sum_kernel<<<balf_ceil_div(kZ * kC, 256), 256, 0, st>>>(l.slab_wd, l.px.S, kZ * kC, dwd_dev);
    BALF_LAUNCH_CHECK();

    // dh[pixel][k] = [a > 0] * sum_c dzT[c][pixel] * Wd[c][k]
    g = GemmArgs{};
    g.A = l.dzT; g.a_sm = 1; g.a_sk = (size_t)N;
    g.B = wd_dev; g.b_sn = 1; g.b_sk = kC;
    g.M = N; g.Nn = kC; g.K = kZ; g.k_rows = kZ;
    g.C = l.dh; g.c_sm = kC; g.mask = l.a;
    launch_gemm<false, false, false, EPI_RELU_MASK>(g, st);
    BALF_LAUNCH_CHECK();
    BALF_TRY(bias_grad(l.dh, kC, kC, l.px, l.b2_part, db2_dev, st));

    // dW2[o][k] = sum_pixel dh[pixel][o] * x2[pixel][k], in S slices of the pixels
    BALF_TRY(weight_grad(l.dh, kC, kC, x2_dev, kC, kC, l.px, l.slab_w2, dw2_dev, st));
    // dx2[pixel][k] = sum_o dh[pixel][o] * W2[o][k]
    return dx2_dev ? pixel_gemm<EPI_STORE, true>(l.dh, kC, kC, w2_dev, kC, N, dx2_dev, kC, nullptr, nullptr, st) : BALF_OK;
}
