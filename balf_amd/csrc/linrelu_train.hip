// balf_linrelu_train_forward / balf_linrelu_train_backward (include/balf_hip.h): a per-pixel Linear c_in -> 2 c_in followed by a ReLU
// in training form,  y = relu(x w^T + b),  and its backward from the total gradient g at y to dw, db and, on request, dx
// (DESIGN.md 7o).  It is the first layer of a Down stage: down4.conv.0 at c_in = 128 (the x0 of balf_forward_gmlp_input), and the
// same layer of stages 2 and 3 at c_in = 32 and 64.  N pixels.
//
//   * forward: gemm_kernel (train_gemm.h) with EPI_BIAS_N_RELU, launched as stage4_input of stage_view.hip launches it: the same
//     MFMA chain, k ascending, and the same epilogue, hence the same bits.
//   * backward: relu_mask_colsum_kernel, the one kernel of this file (its 16-byte accesses are ld4 / st4 of train_gemm.h), makes
//     gm = y > 0 ? g : 0 (the derivative from the OUTPUT, a select) and the float64 column sums of gm per workgroup in one pass:
//     R rows in flight and four columns per thread, another shape than chain4_sum's, so it keeps its own loop; finish_cols adds
//     them to db; dw = gm^T x goes through weight_grad (the K-sliced GEMM and slab_sum_kernel); dx = gm w is one EPI_STORE GEMM,
//     not launched when dx is not wanted.
// No floating-point atomics; every order is a function of (N, c_in) alone.
// workspace: gm [N, c_out] float32, part [P][c_out] float64, slab [S][c_out][c_in] float32.
#include "train_gemm.h"

namespace balf {
namespace {

struct Layout {
    int c_in, c_out;
    PixelSlices px;                         // px.PC workgroups of px.col_rows rows in the mask kernel
    float *gm, *slab;
    double *part;
};

Layout make_layout(int N, int c_in, char *work, size_t *work_bytes) {
    Layout l{};
    l.c_in = c_in; l.c_out = 2 * c_in;
    l.px = pixel_slices(N);
    WorkspaceCursor ws{work, 0};
    l.gm = ws.take<float>((size_t)N * l.c_out * sizeof(float));
    l.part = ws.take<double>((size_t)l.px.PC * l.c_out * sizeof(double));
    l.slab = ws.take<float>((size_t)l.px.S * l.c_out * l.c_in * sizeof(float));
    if (work_bytes) *work_bytes = ws.used;
    return l;
}

// rows [blockIdx.x * rows, ..) of g and y [N,C]: gm = y > 0 ? g : 0, stored, and part[block][c] = the float64 sum of gm's column
// c over these rows.  A thread owns four consecutive columns (one 16-byte load of g and of y, one store of gm per row) of the rows
// r0 + j, r0 + j + R, .. with R = 1024 / C rows in flight per workgroup; its four float64 chains run row ascending, and the R
// chains of a column are then added j ascending through LDS.
template <int C>
__global__ __launch_bounds__(256) void relu_mask_colsum_kernel(const float *g, const float *y, int N, int rows, float *gm, double *part) {
    constexpr int kQuads = C / 4, kR = 256 / kQuads;
    __shared__ double s_sum[kR][C];
    const int q = threadIdx.x % kQuads, j = threadIdx.x / kQuads;
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + j; r < r1; r += kR) {
        const size_t at = (size_t)r * C + 4 * q;
        const gf4 gv = ld4(g + at), yv = ld4(y + at);
        gf4 m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m[i] = yv[i] > 0.0f ? gv[i] : 0.0f;
            s[i] += (double)m[i];
        }
        st4(gm + at, m);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s_sum[j][4 * q + i] = s[i];
    __syncthreads();
    if (threadIdx.x < C) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kR; ++k) v += s_sum[k][threadIdx.x];
        part[(size_t)blockIdx.x * C + threadIdx.x] = v;
    }
}

bool width_ok(int c_in) { return c_in == 32 || c_in == 64 || c_in == 128; }

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" size_t balf_linrelu_train_workspace_bytes(int N, int c_in) {
    if (!width_ok(c_in) || N < 1 || N > kTrainMaxN) return 0;
    size_t bytes = 0;
    make_layout(N, c_in, nullptr, &bytes);
    return bytes;
}

extern "C" int balf_linrelu_train_forward(const float *x_dev, const float *w_dev, const float *b_dev, int N, int c_in, float *y_dev,
                                          void *stream) {
    if (!x_dev || !w_dev || !b_dev || !y_dev || !width_ok(c_in)) return BALF_ERR_ARG;
    if (misaligned(x_dev, 15) || misaligned(w_dev, 15) || misaligned(b_dev, 15) || misaligned(y_dev, 15)) return BALF_ERR_ARG;
    if (N < 1 || N > kTrainMaxN) return BALF_ERR_SHAPE;
    return pixel_gemm<EPI_BIAS_N_RELU, false>(x_dev, c_in, c_in, w_dev, 2 * c_in, N, y_dev, 2 * c_in, b_dev, nullptr,
                                              static_cast<hipStream_t>(stream));
}

extern "C" int balf_linrelu_train_backward(const float *g_dev, const float *y_dev, const float *x_dev, const float *w_dev, int N, int c_in,
                                           float *dw_dev, float *db_dev, float *dx_dev, void *workspace_dev, size_t workspace_bytes,
                                           void *stream) {
    if (!g_dev || !y_dev || !x_dev || !w_dev || !dw_dev || !db_dev || !workspace_dev || !width_ok(c_in)) return BALF_ERR_ARG;
    if (misaligned(g_dev, 15) || misaligned(y_dev, 15) || misaligned(x_dev, 15) || misaligned(w_dev, 15) || misaligned(dw_dev, 15) ||
        misaligned(db_dev, 15) || misaligned(dx_dev, 15) || misaligned(workspace_dev, 15))
        return BALF_ERR_ARG;
    if (N < 1 || N > kTrainMaxN) return BALF_ERR_SHAPE;
    if (workspace_bytes < balf_linrelu_train_workspace_bytes(N, c_in)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout l = make_layout(N, c_in, static_cast<char *>(workspace_dev), nullptr);
    const int c_out = l.c_out;

    // gm = y > 0 ? g : 0 and db = sum gm
    if (c_out == 64) relu_mask_colsum_kernel<64><<<l.px.PC, 256, 0, st>>>(g_dev, y_dev, N, l.px.col_rows, l.gm, l.part);
    else if (c_out == 128) relu_mask_colsum_kernel<128><<<l.px.PC, 256, 0, st>>>(g_dev, y_dev, N, l.px.col_rows, l.gm, l.part);
    else relu_mask_colsum_kernel<256><<<l.px.PC, 256, 0, st>>>(g_dev, y_dev, N, l.px.col_rows, l.gm, l.part);
    BALF_LAUNCH_CHECK();
    BALF_TRY(finish_cols(l.part, c_out, l.px.PC, db_dev, st));
    // dw[o][k] = fl32(sum_pixel gm[pixel][o] * x[pixel][k]) in S slices of the pixels, the slabs added in float64
    BALF_TRY(weight_grad(l.gm, c_out, c_out, x_dev, c_in, c_in, l.px, l.slab, dw_dev, st));
    // dx[pixel][k] = sum_o gm[pixel][o] * w[o][k]
    return dx_dev ? pixel_gemm<EPI_STORE, true>(l.gm, c_out, c_out, w_dev, c_in, N, dx_dev, c_in, nullptr, nullptr, st) : BALF_OK;
}
