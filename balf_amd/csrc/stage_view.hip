// balf_forward_stage_view: the activations that cross the stage boundaries of the detector forward, copied out of the
// forward's workspace as plain fp32 NHWC tensors.  A validation aid, not part of the data path: the reference's forward
// returns only {'logits', 'prob'} (/root/reference/balf/model/mlp_ma_decoder.py:278-285), but its four Down stages are
// separately observable modules (forward hooks on down1..down4), and a wrong kernel should fail at the stage that has it.
#include "det_common.h"
#include "split16.h"
#include "train_gemm.h"

namespace balf {
namespace {

// fragment formats of the split-f16 path (detector_f16.hip: store_frag_px; stage1_f16.h: store_frag32) -> value
__device__ __forceinline__ float frag_value(const char *base, long pix, int C, int c, bool fmt32) {
    const char *p;
    int lo_off;
    if (fmt32) {            // per pixel and K-step of 16 channels 64 B: [hi: lane half 0, 1 x 8 halves][lo: ...]
        const int s = c >> 4, cc = c & 15, g2 = cc >> 3, h = (cc & 7) >> 2, r = cc & 3;
        p = base + pix * (long)C * 4 + s * 64 + h * 16 + (4 * g2 + r) * 2;
        lo_off = 32;
    } else {                // per pixel and K-step of 32 channels 128 B: [hi: lane quarters 0..3 x 8 halves][lo: ...]
        const int ks = c >> 5, cc = c & 31, t = cc >> 4, q = (cc & 15) >> 2, r = cc & 3;
        p = base + pix * (long)C * 4 + ks * 128 + q * 16 + (4 * t + r) * 2;
        lo_off = 64;
    }
    return (float)*reinterpret_cast<const _Float16 *>(p) + (float)*reinterpret_cast<const _Float16 *>(p + lo_off);
}

__global__ void view_frag_kernel(const char *X, long npix, int C, int fmt32, float *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix * C) return;
    out[i] = frag_value(X, i / C, C, (int)(i % C), fmt32 != 0);
}

__global__ void view_x2_kernel(const float *T, const float *R, const float *scale, long per_img, long n, int C, float *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const long img = (i / C) / per_img;
    out[i] = fmaf(T[i], scale[img * C + c], R[i]);
}

// y = r - x0 in place over x0 (balf_forward_rcab_inputs)
__global__ void rcab_y_kernel(const float *r, float *y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = r[i] - y[i];
}

// the checks the three entry points share, in their order, and the forward's plan over a workspace that they only read
int view_plan(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp, Plan *pl) {
    if (precision != BALF_PREC_FP32 && precision != BALF_PREC_FP16) return BALF_ERR_ARG;
    if (Hp <= 0 || Wp <= 0 || Hp % 64 || Wp % 64) return BALF_ERR_SHAPE;
    *pl = make_plan(B, Hp, Wp, const_cast<void *>(workspace_dev));
    if (workspace_bytes < pl->total) return BALF_ERR_WORKSPACE;
    return B > pl->mb ? BALF_ERR_ARG : BALF_OK;                  // only the last micro-batch of a forward is resident
}

// x0[pixel][o] = relu(sum_k x3[pixel][k] * W[o][k] + b[o]) from the resident stage-3 output with the training GEMM; on the split-f16
// path x3 is de-fragmented into scratch first (pixels * 128 floats)
int stage4_input(int precision, const Plan &pl, int B, int Hp, int Wp, const float *conv0_w, const float *conv0_b,
                 float *x0, float *scratch, hipStream_t st) {
    const int C3 = kC[2], C4 = kC[3];
    const size_t pix = (size_t)B * (Hp / 8) * (Wp / 8);
    const float *x3 = pl.X[2];
    if (precision == BALF_PREC_FP16) {
        hipLaunchKernelGGL(view_frag_kernel, dim3((unsigned)((pix * C3 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const char *>(pl.X[2]), (long)pix, C3,
                           kFmt32[3] ? 1 : 0, scratch);
        BALF_LAUNCH_CHECK();
        x3 = scratch;
    }
    return pixel_gemm<EPI_BIAS_N_RELU, false>(x3, C3, C3, conv0_w, C4, (int)pix, x0, C4, conv0_b, nullptr, st);
}

}  // namespace
}  // namespace balf

extern "C" size_t balf_forward_stage_view_numel(int B, int Hp, int Wp, int stage) {
    if (B <= 0 || Hp <= 0 || Wp <= 0 || Hp % 64 || Wp % 64 || stage < 1 || stage > 4) return 0;
    const int sh = stage < 4 ? stage : 3;                       // stages 1-3 pool 2x2, stage 4 keeps its resolution
    return (size_t)B * (Hp >> sh) * (Wp >> sh) * balf::kC[stage - 1];
}

extern "C" int balf_forward_stage_view(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp,
                                       int stage, float *out_dev, void *stream) {
    using namespace balf;
    if (!workspace_dev || !out_dev || B <= 0 || stage < 1 || stage > 4) return BALF_ERR_ARG;
    Plan pl;
    if (const int rc = view_plan(precision, workspace_dev, workspace_bytes, B, Hp, Wp, &pl); rc != BALF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = balf_forward_stage_view_numel(B, Hp, Wp, stage);
    const int C = kC[stage - 1];
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (stage < 4) {
        const char *X = reinterpret_cast<const char *>(pl.X[stage - 1]);
        if (precision == BALF_PREC_FP32) {
            if (hipMemcpyAsync(out_dev, X, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return BALF_ERR_LAUNCH;
        } else {
            hipLaunchKernelGGL(view_frag_kernel, dim3(blocks), dim3(256), 0, st, X, (long)(n / C), C, kFmt32[stage] ? 1 : 0, out_dev);
        }
    } else {
        const long per_img = (long)(Hp / 8) * (Wp / 8);
        hipLaunchKernelGGL(view_x2_kernel, dim3(blocks), dim3(256), 0, st, pl.T, pl.R, pl.scale, per_img, (long)n, C,
                           out_dev);
    }
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// The inputs of stage 4's RCAB for training (balf_rcab_train_forward): r = y + x0 is what the forward keeps (R of the plan), x0 =
// relu(down4.conv.0(stage-3 output)) is computed again here with the training GEMM, and y = r - x0.  The forward kernels and
// their buffers are read, never changed.  Scratch: the stage-3 view (split-f16 path) goes to the front of r_out, x0 to y_out.
extern "C" int balf_forward_rcab_inputs(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp,
                                        const float *conv0_w_dev, const float *conv0_b_dev, float *y_dev, float *r_dev, void *stream) {
    using namespace balf;
    if (!workspace_dev || !conv0_w_dev || !conv0_b_dev || !y_dev || !r_dev || B <= 0) return BALF_ERR_ARG;
    Plan pl;
    if (const int rc = view_plan(precision, workspace_dev, workspace_bytes, B, Hp, Wp, &pl); rc != BALF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * (Hp / 8) * (Wp / 8) * kC[3];
    const int rc = stage4_input(precision, pl, B, Hp, Wp, conv0_w_dev, conv0_b_dev, y_dev, r_dev, st);
    if (rc != BALF_OK) return rc;
    if (hipMemcpyAsync(r_dev, pl.R, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return BALF_ERR_LAUNCH;
    hipLaunchKernelGGL(rcab_y_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r_dev, y_dev, n);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// The input of stage 4's gMLP layer for training (balf_gmlp_train_forward): x0, the first half of balf_forward_rcab_inputs.
extern "C" int balf_forward_gmlp_input(int precision, const void *workspace_dev, size_t workspace_bytes, int B, int Hp, int Wp,
                                       const float *conv0_w_dev, const float *conv0_b_dev, float *x0_dev, float *scratch_dev,
                                       void *stream) {
    using namespace balf;
    if (!workspace_dev || !conv0_w_dev || !conv0_b_dev || !x0_dev || B <= 0) return BALF_ERR_ARG;
    if (precision == BALF_PREC_FP16 && !scratch_dev) return BALF_ERR_ARG;
    Plan pl;
    if (const int rc = view_plan(precision, workspace_dev, workspace_bytes, B, Hp, Wp, &pl); rc != BALF_OK) return rc;
    return stage4_input(precision, pl, B, Hp, Wp, conv0_w_dev, conv0_b_dev, x0_dev, scratch_dev, (hipStream_t)stream);
}
