// balf_rcab_train_forward_c / balf_rcab_train_backward_c (include/balf_hip.h): a Down stage's ResidualChannelAttentionBlock in
// training form at C channels, C = 256 (stage 4) or 128 (stage 3) a template value of every kernel and of the Layout,
// y -> LayerNorm -> conv1 (Linear C -> C) -> LeakyReLU(0.2) -> conv2 (Linear C -> C) -> squeeze-excite scale (C / 4 hidden units),
// x2 = t * s_image + r,  and its backward from dx2 to the ten parameter gradients and dy.  N = B * Hc * Wc
// pixels.  The C = 256 instantiation is the code that served stage 4 alone: the same operations in the same order.
//
// Four kinds of kernels:
//   * gemm_kernel (train_gemm.h, with its launch helpers) for the six C x C products; dwc1 / dwc2 through the slab split
//     and the float64 slab sum.
//   * LayerNorm row kernels (train_ln.h, shared with gmlp_train.hip): a pixel's C channels on C / 4 lanes; the backward is
//     LN_DX_ADD (dy = dx2 + LN'(dn), dx2 and dy at any 4-byte alignment) or LN_DX_NONE when dy is not asked for.
//   * column kernels, a channel per thread (workgroups of C threads) over a block of pixel rows, float64 partial sums per
//     workgroup, each a term of its own inside chain4_sum (train_gemm.h): over the rows of ONE image (img_sum_kernel: the SE mean m_i and ds_i = sum g t; the grid is
//     (row blocks of an image, image), so no block ever holds rows of two images, wherever an image starts), and over all rows
//     (dt_kernel; col_sum_kernel through bias_grad; ln_bwd_kernel, which has its own row walk).
//   * the squeeze-excite arithmetic in float64: se_fwd_kernel / se_bwd_kernel, a workgroup per image, and se_wgrad_kernel, a
//     thread per element of dws0 / dws2 / dbs0 / dbs2 that walks the images in image order.
// No floating-point atomics; every order is a function of (B, Hc, Wc) alone.
// saved: n, a, t [N,C], (mean, rstd) [N,2], and per image m [C], e [C / 4], s [C] as float64 plus s as float32.
#include "train_ln.h"

namespace balf {
namespace {

constexpr int kMaxImgParts = 1024;          // row blocks per image of img_sum_kernel

struct Layout {
    int B, hw;
    PixelSlices px;                         // of all N = B * hw pixels
    int img_rows, PI;                       // PI blocks of img_rows rows per image
    // saved
    float *n, *a, *t, *stat, *sf;           // stat [N][2]: mean, rstd; sf [B][C]
    double *m, *e, *s;                      // [B][C], [B][C / 4], [B][C]
    // workspace
    double *img_part;                       // [B][PI][C]
    double *col_part;                       // [2][PC][C]
    double *dq, *de;                        // [B][C], [B][C / 4]
    float *dmh;                             // [B][C]: dm / (Hc * Wc)
    float *dt, *dh, *slab;                  // dt [N,C], later dn; dh [N,C]; slab [S][C][C]
};

template <int kC>
Layout make_layout(int B, int hw, char *saved, char *work, size_t *saved_bytes, size_t *work_bytes) {
    constexpr int kH = kC / 4;
    Layout l{};
    l.B = B; l.hw = hw;
    const int N = B * hw;
    l.px = pixel_slices(N);
    const int per = balf_ceil_div(hw, kMaxImgParts);
    l.img_rows = per > 64 ? per : 64;
    l.PI = balf_ceil_div(hw, l.img_rows);
    const size_t act = (size_t)N * kC * sizeof(float);
    WorkspaceCursor sv{saved, 0};
    l.n = sv.take<float>(act);
    l.a = sv.take<float>(act);
    l.t = sv.take<float>(act);
    l.stat = sv.take<float>((size_t)N * 2 * sizeof(float));
    l.m = sv.take<double>((size_t)B * kC * sizeof(double));
    l.e = sv.take<double>((size_t)B * kH * sizeof(double));
    l.s = sv.take<double>((size_t)B * kC * sizeof(double));
    l.sf = sv.take<float>((size_t)B * kC * sizeof(float));
    if (saved_bytes) *saved_bytes = sv.used;
    WorkspaceCursor ws{work, 0};
    l.img_part = ws.take<double>((size_t)B * l.PI * kC * sizeof(double));
    l.col_part = ws.take<double>((size_t)2 * l.px.PC * kC * sizeof(double));
    l.dq = ws.take<double>((size_t)B * kC * sizeof(double));
    l.de = ws.take<double>((size_t)B * kH * sizeof(double));
    l.dmh = ws.take<float>((size_t)B * kC * sizeof(float));
    l.dt = ws.take<float>(act);
    l.dh = ws.take<float>(act);
    l.slab = ws.take<float>((size_t)l.px.S * kC * kC * sizeof(float));
    if (work_bytes) *work_bytes = ws.used;
    return l;
}

// ---- sums over the pixels of one image ----------------------------------------------------------------------------------------
// part[image][block][c] = float64 sum over rows [block * rows, ..) OF THE IMAGE of x[row][c] (PROD: x * w, the product in
// float64, where it is exact); grid (PI, B), a column per thread
template <int kC, bool PROD>
__global__ __launch_bounds__(kC) void img_sum_kernel(const float *x, const float *w, int hw, int rows, double *part) {
    const int img = blockIdx.y;
    const int o0 = blockIdx.x * rows, o1 = min(hw, o0 + rows);
    const size_t base = (size_t)img * (size_t)hw;
    part[((size_t)img * gridDim.x + blockIdx.x) * kC + threadIdx.x] = chain4_sum(o0, o1, [&](int o) {
        const size_t at = (base + o) * kC + threadIdx.x;
        return PROD ? (double)x[at] * (double)w[at] : (double)x[at];
    });
}

struct SeArgs {
    int hw, PI;
    const double *img_part;
    const float *ws0, *bs0, *ws2, *bs2;
    double *m, *e, *s, *dq, *de;
    float *sf, *dmh;
};

template <int kC>
__device__ __forceinline__ double img_part_sum(const SeArgs &a, int img, int c) {
    double v = 0.0;
    for (int k = 0; k < a.PI; ++k) v += a.img_part[((size_t)img * a.PI + k) * kC + c];
    return v;
}

// a workgroup per image: m = mean t, e = relu(m ws0^T + bs0), s = sigmoid(e ws2^T + bs2), float64, k ascending
template <int kC>
__global__ __launch_bounds__(kC) void se_fwd_kernel(SeArgs a) {
    constexpr int kH = kC / 4;
    __shared__ double s_m[kC], s_e[kH];
    const int img = blockIdx.x, c = threadIdx.x;
    const double m = img_part_sum<kC>(a, img, c) / (double)a.hw;
    s_m[c] = m;
    a.m[(size_t)img * kC + c] = m;
    __syncthreads();
    if (c < kH) {
        double v = 0.0;
        for (int k = 0; k < kC; ++k) v += s_m[k] * (double)a.ws0[c * kC + k];
        v += (double)a.bs0[c];
        v = v > 0.0 ? v : 0.0;
        s_e[c] = v;
        a.e[(size_t)img * kH + c] = v;
    }
    __syncthreads();
    double v = 0.0;
    for (int j = 0; j < kH; ++j) v += s_e[j] * (double)a.ws2[c * kH + j];
    v += (double)a.bs2[c];
    const double s = 1.0 / (1.0 + exp(-v));
    a.s[(size_t)img * kC + c] = s;
    a.sf[(size_t)img * kC + c] = (float)s;
}

// a workgroup per image: ds = sum g t, dq = ds s (1 - s), de = (dq ws2) [e > 0], dm = de ws0 -> dq, de, dm / hw
template <int kC>
__global__ __launch_bounds__(kC) void se_bwd_kernel(SeArgs a) {
    constexpr int kH = kC / 4;
    __shared__ double s_q[kC], s_e[kH];
    const int img = blockIdx.x, c = threadIdx.x;
    const double s = a.s[(size_t)img * kC + c];
    const double dq = img_part_sum<kC>(a, img, c) * s * (1.0 - s);
    s_q[c] = dq;
    a.dq[(size_t)img * kC + c] = dq;
    __syncthreads();
    if (c < kH) {
        double v = 0.0;
        for (int k = 0; k < kC; ++k) v += s_q[k] * (double)a.ws2[k * kH + c];
        v = a.e[(size_t)img * kH + c] > 0.0 ? v : 0.0;
        s_e[c] = v;
        a.de[(size_t)img * kH + c] = v;
    }
    __syncthreads();
    double v = 0.0;
    for (int j = 0; j < kH; ++j) v += s_e[j] * (double)a.ws0[j * kC + c];
    a.dmh[(size_t)img * kC + c] = (float)(v / (double)a.hw);
}

struct SeGradArgs {
    int B;
    const double *dq, *de, *m, *e;
    float *dws0, *dbs0, *dws2, *dbs2;
};

// a thread per output element, the images in image order: dws2 = sum dq^T e, dws0 = sum de^T m, dbs2 = sum dq, dbs0 = sum de
template <int kC>
__global__ __launch_bounds__(256) void se_wgrad_kernel(SeGradArgs a) {
    constexpr int kH = kC / 4;
    int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < kC * kH) {
        const int c = i / kH, j = i - c * kH;
        for (int b = 0; b < a.B; ++b) v += a.dq[(size_t)b * kC + c] * a.e[(size_t)b * kH + j];
        a.dws2[i] = (float)v;
        return;
    }
    i -= kC * kH;
    if (i < kH * kC) {
        const int j = i / kC, c = i - j * kC;
        for (int b = 0; b < a.B; ++b) v += a.de[(size_t)b * kH + j] * a.m[(size_t)b * kC + c];
        a.dws0[i] = (float)v;
        return;
    }
    i -= kH * kC;
    if (i < kC) {
        for (int b = 0; b < a.B; ++b) v += a.dq[(size_t)b * kC + i];
        a.dbs2[i] = (float)v;
        return;
    }
    i -= kC;
    if (i < kH) {
        for (int b = 0; b < a.B; ++b) v += a.de[(size_t)b * kH + i];
        a.dbs0[i] = (float)v;
    }
}

// ---- element kernels ----------------------------------------------------------------------------------------------------------
// x2 = fma(t, s_image, r), four channels per thread
template <int kC>
__global__ __launch_bounds__(256) void scale_add_kernel(const float *t, const float *sf, const float *r, size_t quads, int hw, float *x2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const size_t p = i / (kC / 4);
    const int c = 4 * (int)(i - p * (kC / 4));
    const gf4 tv = ld4(t + 4 * i), rv = ld4(r + 4 * i), sv = ld4(sf + (p / (size_t)hw) * kC + c);
    gf4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(tv[j], sv[j], rv[j]);
    st4(x2 + 4 * i, o);
}

// rows [blockIdx.x * rows, ..) of the pixels, a column per thread: dt = fma(g, s_image, dm_image / hw), stored, and its float64
// column sums (dbc2) as this block's partial
template <int kC>
__global__ __launch_bounds__(kC) void dt_kernel(const float *g, const float *sf, const float *dmh, int N, int hw, int rows, float *dt,
                                                double *part) {
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows), c = threadIdx.x;
    part[(size_t)blockIdx.x * kC + c] = chain4_sum(r0, r1, [&](int r) {
        const size_t at = (size_t)r * kC + c, im = (size_t)(r / hw) * kC + c;
        const float v = fmaf(g[at], sf[im], dmh[im]);
        dt[at] = v;
        return (double)v;
    });
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
template <int kC>
size_t layout_bytes(int B, int Hc, int Wc, bool saved) {
    size_t sv = 0, ws = 0;
    make_layout<kC>(B, Hc * Wc, nullptr, nullptr, &sv, &ws);
    return saved ? sv : ws;
}

template <int kC>
int rcab_forward(const float *y_dev, const float *r_dev, const float *ln_g_dev, const float *ln_b_dev, const float *wc1_dev,
                 const float *bc1_dev, const float *wc2_dev, const float *bc2_dev, const float *ws0_dev, const float *bs0_dev,
                 const float *ws2_dev, const float *bs2_dev, int B, int Hc, int Wc, float *x2_dev, void *saved_dev, void *workspace_dev,
                 size_t workspace_bytes, void *stream) {
    if (!y_dev || !r_dev || !ln_g_dev || !ln_b_dev || !wc1_dev || !bc1_dev || !wc2_dev || !bc2_dev || !ws0_dev || !bs0_dev || !ws2_dev ||
        !bs2_dev || !x2_dev || !saved_dev || !workspace_dev)
        return BALF_ERR_ARG;
    // 16-byte loads and stores of whole channel quads; the float64 blocks of saved and workspace
    if (misaligned(y_dev, 15) || misaligned(r_dev, 15) || misaligned(x2_dev, 15) || misaligned(ln_g_dev, 15) || misaligned(ln_b_dev, 15) ||
        misaligned(saved_dev, 15) || misaligned(workspace_dev, 15))
        return BALF_ERR_ARG;
    const int rc = check_sizes(B, Hc, Wc);
    if (rc != BALF_OK) return rc;
    if (workspace_bytes < layout_bytes<kC>(B, Hc, Wc, false)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = Hc * Wc, N = B * hw;
    const Layout l = make_layout<kC>(B, hw, static_cast<char *>(saved_dev), static_cast<char *>(workspace_dev), nullptr, nullptr);

    BALF_TRY(ln_forward<kC>(y_dev, kC, ln_g_dev, ln_b_dev, N, l.n, l.stat, st));
    BALF_TRY((pixel_gemm<EPI_BIAS_N_LRELU, false>(l.n, kC, kC, wc1_dev, kC, N, l.a, kC, bc1_dev, nullptr, st)));   // a = lrelu(n wc1^T + bc1)
    BALF_TRY((pixel_gemm<EPI_BIAS_N, false>(l.a, kC, kC, wc2_dev, kC, N, l.t, kC, bc2_dev, nullptr, st)));         // t = a wc2^T + bc2
    img_sum_kernel<kC, false><<<dim3(l.PI, B), kC, 0, st>>>(l.t, nullptr, hw, l.img_rows, l.img_part);
    BALF_LAUNCH_CHECK();
    SeArgs s{};
    s.hw = hw; s.PI = l.PI; s.img_part = l.img_part;
    s.ws0 = ws0_dev; s.bs0 = bs0_dev; s.ws2 = ws2_dev; s.bs2 = bs2_dev;
    s.m = l.m; s.e = l.e; s.s = l.s; s.sf = l.sf;
    se_fwd_kernel<kC><<<B, kC, 0, st>>>(s);
    BALF_LAUNCH_CHECK();
    const size_t quads = (size_t)N * (kC / 4);
    scale_add_kernel<kC><<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(l.t, l.sf, r_dev, quads, hw, x2_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

template <int kC>
int rcab_backward(const float *dx2_dev, const float *y_dev, const float *ln_g_dev, const float *wc1_dev, const float *wc2_dev,
                  const float *ws0_dev, const float *ws2_dev, const void *saved_dev, int B, int Hc, int Wc, float *dln_g_dev,
                  float *dln_b_dev, float *dwc1_dev, float *dbc1_dev, float *dwc2_dev, float *dbc2_dev, float *dws0_dev, float *dbs0_dev,
                  float *dws2_dev, float *dbs2_dev, float *dy_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!dx2_dev || !y_dev || !ln_g_dev || !wc1_dev || !wc2_dev || !ws0_dev || !ws2_dev || !saved_dev || !dln_g_dev || !dln_b_dev ||
        !dwc1_dev || !dbc1_dev || !dwc2_dev || !dbc2_dev || !dws0_dev || !dbs0_dev || !dws2_dev || !dbs2_dev || !workspace_dev)
        return BALF_ERR_ARG;
    if (misaligned(y_dev, 15) || misaligned(ln_g_dev, 15) || misaligned(saved_dev, 15) || misaligned(workspace_dev, 15)) return BALF_ERR_ARG;
    const int rc = check_sizes(B, Hc, Wc);
    if (rc != BALF_OK) return rc;
    if (workspace_bytes < layout_bytes<kC>(B, Hc, Wc, false)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = Hc * Wc, N = B * hw;
    const Layout l = make_layout<kC>(B, hw, static_cast<char *>(const_cast<void *>(saved_dev)), static_cast<char *>(workspace_dev), nullptr,
                                 nullptr);
    double *part0 = l.col_part, *part1 = l.col_part + (size_t)l.px.PC * kC;

    // the squeeze-excite: ds_i = sum_p g t, then dq, de, dm per image and the four SE gradients over the images
    img_sum_kernel<kC, true><<<dim3(l.PI, B), kC, 0, st>>>(dx2_dev, l.t, hw, l.img_rows, l.img_part);
    BALF_LAUNCH_CHECK();
    SeArgs s{};
    s.hw = hw; s.PI = l.PI; s.img_part = l.img_part;
    s.ws0 = ws0_dev; s.ws2 = ws2_dev;
    s.m = l.m; s.e = l.e; s.s = l.s; s.sf = l.sf; s.dq = l.dq; s.de = l.de; s.dmh = l.dmh;
    se_bwd_kernel<kC><<<B, kC, 0, st>>>(s);
    BALF_LAUNCH_CHECK();
    SeGradArgs sg{};
    sg.B = B; sg.dq = l.dq; sg.de = l.de; sg.m = l.m; sg.e = l.e;
    sg.dws0 = dws0_dev; sg.dbs0 = dbs0_dev; sg.dws2 = dws2_dev; sg.dbs2 = dbs2_dev;
    se_wgrad_kernel<kC><<<balf_ceil_div(2 * kC * (kC / 4) + kC + kC / 4, 256), 256, 0, st>>>(sg);
    BALF_LAUNCH_CHECK();

    // dt = g s_i + dm_i / hw, dbc2 = sum dt, dwc2 = dt^T a
    dt_kernel<kC><<<l.px.PC, kC, 0, st>>>(dx2_dev, l.sf, l.dmh, N, hw, l.px.col_rows, l.dt, part0);
    BALF_LAUNCH_CHECK();
    BALF_TRY(finish_cols(part0, kC, l.px.PC, dbc2_dev, st));
    BALF_TRY(weight_grad(l.dt, kC, kC, l.a, kC, kC, l.px, l.slab, dwc2_dev, st));
    // dh = (dt wc2) * (a > 0 ? 1 : 0.2), dbc1 = sum dh, dwc1 = dh^T n
    BALF_TRY((pixel_gemm<EPI_LRELU_MASK, true>(l.dt, kC, kC, wc2_dev, kC, N, l.dh, kC, nullptr, l.a, st)));
    BALF_TRY(bias_grad(l.dh, kC, kC, l.px, part0, dbc1_dev, st));
    BALF_TRY(weight_grad(l.dh, kC, kC, l.n, kC, kC, l.px, l.slab, dwc1_dev, st));
    // dn = dh wc1 (over dt, which nobody reads any more), then the LayerNorm: dln_g, dln_b and, if asked for, dy = dx2 + LN'(dn)
    float *dn = l.dt;
    BALF_TRY((pixel_gemm<EPI_STORE, true>(l.dh, kC, kC, wc1_dev, kC, N, dn, kC, nullptr, nullptr, st)));
    LnBwdArgs b{};
    b.dn = dn; b.stat = l.stat; b.ln_g = ln_g_dev; b.x = y_dev; b.xs = kC; b.g = dx2_dev; b.gs = kC; b.out = dy_dev; b.os = kC;
    b.part_g = part0; b.part_b = part1;
    b.vec_g = !misaligned(dx2_dev, 15); b.vec_out = !misaligned(dy_dev, 15);
    return dy_dev ? ln_backward<kC, LN_DX_ADD>(b, l.px, dln_g_dev, dln_b_dev, st)
                  : ln_backward<kC, LN_DX_NONE>(b, l.px, dln_g_dev, dln_b_dev, st);
}

}  // namespace

// the unit's two sizes for balf_train_unit_sizes (train_sizes.hip): the code of the size check, and the outputs only with BALF_OK
int rcab_train_sizes(int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    BALF_TRY(check_sizes(B, Hc, Wc));
    *workspace_bytes = C == 128 ? layout_bytes<128>(B, Hc, Wc, false) : layout_bytes<256>(B, Hc, Wc, false);
    *saved_bytes = C == 128 ? layout_bytes<128>(B, Hc, Wc, true) : layout_bytes<256>(B, Hc, Wc, true);
    return BALF_OK;
}

}  // namespace balf

using namespace balf;

extern "C" size_t balf_rcab_train_workspace_bytes(int B, int Hc, int Wc) {
    return check_sizes(B, Hc, Wc) == BALF_OK ? layout_bytes<256>(B, Hc, Wc, false) : 0;
}

extern "C" size_t balf_rcab_train_saved_bytes(int B, int Hc, int Wc) {
    return check_sizes(B, Hc, Wc) == BALF_OK ? layout_bytes<256>(B, Hc, Wc, true) : 0;
}

extern "C" int balf_rcab_train_forward_c(const float *y_dev, const float *r_dev, const float *ln_g_dev, const float *ln_b_dev,
                                         const float *wc1_dev, const float *bc1_dev, const float *wc2_dev, const float *bc2_dev,
                                         const float *ws0_dev, const float *bs0_dev, const float *ws2_dev, const float *bs2_dev, int B,
                                         int Hc, int Wc, int C, float *x2_dev, void *saved_dev, void *workspace_dev,
                                         size_t workspace_bytes, void *stream) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    return (C == 128 ? rcab_forward<128> : rcab_forward<256>)(y_dev, r_dev, ln_g_dev, ln_b_dev, wc1_dev, bc1_dev, wc2_dev, bc2_dev, ws0_dev,
                                                              bs0_dev, ws2_dev, bs2_dev, B, Hc, Wc, x2_dev, saved_dev, workspace_dev,
                                                              workspace_bytes, stream);
}

extern "C" int balf_rcab_train_backward_c(const float *dx2_dev, const float *y_dev, const float *ln_g_dev, const float *wc1_dev,
                                          const float *wc2_dev, const float *ws0_dev, const float *ws2_dev, const void *saved_dev, int B,
                                          int Hc, int Wc, int C, float *dln_g_dev, float *dln_b_dev, float *dwc1_dev, float *dbc1_dev,
                                          float *dwc2_dev, float *dbc2_dev, float *dws0_dev, float *dbs0_dev, float *dws2_dev,
                                          float *dbs2_dev, float *dy_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    return (C == 128 ? rcab_backward<128> : rcab_backward<256>)(dx2_dev, y_dev, ln_g_dev, wc1_dev, wc2_dev, ws0_dev, ws2_dev, saved_dev, B,
                                                                Hc, Wc, dln_g_dev, dln_b_dev, dwc1_dev, dbc1_dev, dwc2_dev, dbc2_dev,
                                                                dws0_dev, dbs0_dev, dws2_dev, dbs2_dev, dy_dev, workspace_dev,
                                                                workspace_bytes, stream);
}

extern "C" int balf_rcab_train_forward(const float *y_dev, const float *r_dev, const float *ln_g_dev, const float *ln_b_dev,
                                       const float *wc1_dev, const float *bc1_dev, const float *wc2_dev, const float *bc2_dev,
                                       const float *ws0_dev, const float *bs0_dev, const float *ws2_dev, const float *bs2_dev, int B,
                                       int Hc, int Wc, float *x2_dev, void *saved_dev, void *workspace_dev, size_t workspace_bytes,
                                       void *stream) {
    return balf_rcab_train_forward_c(y_dev, r_dev, ln_g_dev, ln_b_dev, wc1_dev, bc1_dev, wc2_dev, bc2_dev, ws0_dev, bs0_dev, ws2_dev, bs2_dev,
                                     B, Hc, Wc, 256, x2_dev, saved_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int balf_rcab_train_backward(const float *dx2_dev, const float *y_dev, const float *ln_g_dev, const float *wc1_dev,
                                        const float *wc2_dev, const float *ws0_dev, const float *ws2_dev, const void *saved_dev, int B,
                                        int Hc, int Wc, float *dln_g_dev, float *dln_b_dev, float *dwc1_dev, float *dbc1_dev,
                                        float *dwc2_dev, float *dbc2_dev, float *dws0_dev, float *dbs0_dev, float *dws2_dev,
                                        float *dbs2_dev, float *dy_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return balf_rcab_train_backward_c(dx2_dev, y_dev, ln_g_dev, wc1_dev, wc2_dev, ws0_dev, ws2_dev, saved_dev, B, Hc, Wc, 256, dln_g_dev,
                                      dln_b_dev, dwc1_dev, dbc1_dev, dwc2_dev, dbc2_dev, dws0_dev, dbs0_dev, dws2_dev, dbs2_dev, dy_dev,
                                      workspace_dev, workspace_bytes, stream);
}
