// balf_gmlp_train_forward_c / balf_gmlp_train_backward_c (include/balf_hip.h): a Down stage's ResidualSplitHeadMultiAxisGmlpLayer
// in training form at C channels, C = 256 (stage 4) or 128 (stage 3) a template value of every kernel and of the Layout; the text
// below writes the widths of C = 256, and 256 / 512 read C / 2C throughout.
// x0 -> LayerNorm -> dense1 (256 -> 512) -> GELU -> halves (u, v) -> the grid branch on u, the block branch on v
// -> dense2 (512 -> 256) + x0 = y,  and its backward from dy to the 26 parameter gradients and dx0.
// N = B * Hc * Wc pixels.  A branch on z [N,256]:  LayerNorm -> dense1 (256 -> 512) -> GELU -> halves (a, c) -> LayerNorm of c ->
// the 64 x 64 product along the TOKEN axis -> gate a * (mix + 1) -> dense2 (256 -> 256) + z.
// The C = 256 instantiation is the code that served stage 4 alone: the same operations in the same order.
//
// Kernels:
//   * gemm_kernel (train_gemm.h) for every product along the channels; GELU is its epilogue EPI_BIAS_N_GELU, which also keeps the
//     pre-activation, the shortcuts are EPI_BIAS_N_ADD.  The weight gradients go through the slab split and the float64 slab sum.
//   * LayerNorm: ln_fwd_kernel / ln_bwd_kernel of train_ln.h for all five norms.  The layer's own reads rows of x0 [N,256]
//     (LN_DX_ADD, or LN_DX_NONE without dx0); the four of the branches read a 256-channel half of a [N,512] row (row stride 512,
//     the column offset in the pointer), and their backward multiplies by the GELU derivative of the product that made its input
//     (LN_DX_GELU, LN_DX_ADD_GELU), so that dH = dG * gelu'(H) costs no pass of its own.
//   * the token mix.  A group's 64 tokens are 64 pixels that no single stride addresses: pixel(token) = base(group) +
//     (token >> 3) * sy + (token & 7) * sx, with (sy, sx) = (Hc / 8 * Wc, Wc / 8) under the grid map and (Wc, 1) under the block
//     map.  mix_fwd_kernel / mix_bwd_kernel take a workgroup per group, Wt in LDS, and gather the rows through that map: wave w
//     owns channels 64 w .. 64 w + 63 of all 64 tokens, a lane loads four consecutive channels of a token's row straight into the
//     B operands of four MFMA tiles (tile j, column li <-> channel 64 w + 4 li + j), so every activation is read once, by one
//     lane, as a 16-byte load, and nothing is transposed through memory.  k, the token summed over, ascends.
//   * column sums in float64 per workgroup of rows (bias_grad: col_sum_kernel over 256 or 512 columns of a row of stride 256 or
//     512), added by partial_sum_kernel.
// dWt and dbt: each wave of mix_bwd_kernel sums dmix cn^T over its 64 channels in an MFMA chain per group and adds the groups of
// its workgroup in float64 registers; the (C / 64) * PW wave partials (a workgroup has C / 64 waves, one per 64 channels: C
// threads) are added by partial_sum_kernel in one fixed order.
// No floating-point atomics; every order is a function of (B, Hc, Wc) alone.
#include "train_ln.h"

namespace balf {
namespace {

constexpr int kTok = 64;                    // tokens of a group: the 8 x 8 grid, the 8 x 8 block
constexpr int kParams = 26;
constexpr int kBranchParams = 10;           // norm.{w,b} dense1.{w,b} gating norm.{w,b} gating dense.{w,b} dense2.{w,b}
constexpr int kMixPitch = 80;               // floats per row of Wt in LDS: the four k of an MFMA step fall on disjoint banks
constexpr int kMixPart = kTok * kTok + kTok;    // float64 per wave partial: dWt, then dbt
constexpr int kMaxMixWgs = 256;             // workgroups of mix_bwd_kernel: one per CU, or one per group when there are fewer

struct Branch {                             // saved, per branch
    float *nb, *statb, *hb, *gb, *statg, *cn, *mixp1, *gated;
};

struct Layout {
    int B, Hc, Wc, groups, gpw, PW;
    PixelSlices px;
    // saved
    float *n0, *stat0, *h0, *g0, *cat;
    Branch br[2];
    // workspace
    double *col_part;                       // [2][PC][512]
    double *mix_part;                       // [(C / 64) PW][kMixPart]
    float *dcat, *dh0, *dhb;                // [N,512] each
    float *t0, *t1;                         // [N,256]: dgated, then dnb, then dn0; dcn
    float *slab;                            // [S][512 * 256]
};

template <int kC>
Layout make_layout(int B, int Hc, int Wc, char *saved, char *work, size_t *saved_bytes, size_t *work_bytes) {
    constexpr int kC2 = 2 * kC;             // the width of the two dense1 outputs and of the concatenation
    Layout l{};
    l.B = B; l.Hc = Hc; l.Wc = Wc;
    const int N = B * Hc * Wc;
    l.px = pixel_slices(N);
    l.groups = N / kTok;
    l.gpw = balf_ceil_div(l.groups, kMaxMixWgs);
    l.PW = balf_ceil_div(l.groups, l.gpw);
    const size_t a1 = (size_t)N * kC * sizeof(float), a2 = 2 * a1, st = (size_t)N * 2 * sizeof(float);
    WorkspaceCursor sv{saved, 0};
    l.n0 = sv.take<float>(a1);
    l.stat0 = sv.take<float>(st);
    l.h0 = sv.take<float>(a2);
    l.g0 = sv.take<float>(a2);
    l.cat = sv.take<float>(a2);
    for (Branch &b : l.br) {
        b.nb = sv.take<float>(a1);
        b.statb = sv.take<float>(st);
        b.hb = sv.take<float>(a2);
        b.gb = sv.take<float>(a2);
        b.statg = sv.take<float>(st);
        b.cn = sv.take<float>(a1);
        b.mixp1 = sv.take<float>(a1);
        b.gated = sv.take<float>(a1);
    }
    if (saved_bytes) *saved_bytes = sv.used;
    WorkspaceCursor ws{work, 0};
    l.col_part = ws.take<double>((size_t)2 * l.px.PC * kC2 * sizeof(double));
    l.mix_part = ws.take<double>((size_t)(kC / 64) * l.PW * kMixPart * sizeof(double));
    l.dcat = ws.take<float>(a2);
    l.dh0 = ws.take<float>(a2);
    l.dhb = ws.take<float>(a2);
    l.t0 = ws.take<float>(a1);
    l.t1 = ws.take<float>(a1);
    l.slab = ws.take<float>((size_t)l.px.S * kC2 * kC * sizeof(float));
    if (work_bytes) *work_bytes = ws.used;
    return l;
}

// ---- the token mix -------------------------------------------------------------------------------------------------------------
struct MixArgs {
    int groups, gpw;                        // groups in all; per workgroup of the backward
    int per_img, fw, HW, by, bx, sy, sx;    // base(group) = image * HW + iy * by + ix * bx, (iy, ix) = the group's place in its image
    const float *wt, *bt;                   // [64,64], [64]
    const float *cn, *gb;                   // LayerNorm(c) [N,256]; gelu(hb) [N,512], a = its lower half
    float *mixp1, *gated;                   // forward: mix + 1, a * (mix + 1)  [N,256]
    const float *dgated, *hb, *mixp1_in;    // backward
    float *dhb, *dcn;                       // dhb [N,512], its lower half written here; dcn [N,256]
    double *part;                           // [(C / 64) * PW][kMixPart]
};

__device__ __forceinline__ size_t group_base(const MixArgs &a, int g) {
    const int img = g / a.per_img, rem = g - img * a.per_img, iy = rem / a.fw, ix = rem - iy * a.fw;
    return (size_t)img * a.HW + (size_t)iy * a.by + (size_t)ix * a.bx;
}
__device__ __forceinline__ size_t token_pixel(const MixArgs &a, size_t base, int t) {
    return base + (size_t)((t >> 3) * a.sy + (t & 7) * a.sx);
}

typedef float (*MixTile)[kMixPitch];

// TRANSPOSE: sW[q][p] = Wt[p][q] (forward: the MFMA's A operand is (m = p, k = q)); else sW[p][q] (backward: (m = q, k = p))
template <int kC, bool TRANSPOSE>
__device__ __forceinline__ void load_wt(const float *wt, MixTile sW) {
    for (int e = threadIdx.x; e < kTok * kTok; e += kC) {   // (a workgroup of kC threads)
        const int p = e >> 6, q = e & 63;
        if (TRANSPOSE) sW[q][p] = wt[e];
        else sW[p][q] = wt[e];
    }
}

__device__ __forceinline__ void zero_acc(gf4 (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gf4{0.0f, 0.0f, 0.0f, 0.0f};
}

// a workgroup per group: mix[p][ch] = sum_q Wt[p][q] cn[q][ch] + bt[p], q ascending; mixp1 = mix + 1; gated = a * mixp1
template <int kC>
__global__ __launch_bounds__(kC) void mix_fwd_kernel(MixArgs a) {
    constexpr int kC2 = 2 * kC;
    __shared__ float sW[kTok][kMixPitch];
    __shared__ float sB[kTok];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
    load_wt<kC, true>(a.wt, sW);
    if (threadIdx.x < kTok) sB[threadIdx.x] = a.bt[threadIdx.x];
    __syncthreads();
    const size_t base = group_base(a, blockIdx.x);
    const int ch = 64 * wave + 4 * li;
    gf4 acc[4][4];
    zero_acc(acc);
#pragma unroll 4
    for (int ks = 0; ks < kTok / 4; ++ks) {
        const int k = 4 * ks + q;
        const gf4 b = ld4(a.cn + token_pixel(a, base, k) * kC + ch);
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = sW[k][16 * i + li];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], b[j], acc[i][j], 0, 0, 0);
    }
    // tile (i, j), register r: token 16 i + 4 q + r, channel ch + j
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * i + 4 * q + r;
            const size_t pix = token_pixel(a, base, m);
            const float bias = sB[m];
            const gf4 av = ld4(a.gb + pix * kC2 + ch);
            gf4 mp, gt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mp[j] = (acc[i][j][r] + bias) + 1.0f;
                gt[j] = av[j] * mp[j];
            }
            st4(a.mixp1 + pix * kC + ch, mp);
            st4(a.gated + pix * kC + ch, gt);
        }
}

// a workgroup per gpw consecutive groups.  Per group: dmix = dgated * a;  dhb(lower half) = dgated * mixp1 * gelu'(hb);
// dcn[q][ch] = sum_p Wt[p][q] dmix[p][ch], p ascending;  then, over the wave's own 64 channels, dWt[p][q] += sum_ch dmix[p][ch]
// cn[q][ch] (lane quarter k of step s takes channel 16 k + s of the 64: four 16-byte loads cover the sixteen steps) and dbt[p] +=
// sum_ch dmix[p][ch].  The groups of the workgroup are added in float64 registers, in group order.
template <int kC>
__global__ __launch_bounds__(kC) void mix_bwd_kernel(MixArgs a) {
    constexpr int kC2 = 2 * kC;
    __shared__ float sW[kTok][kMixPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
    load_wt<kC, false>(a.wt, sW);
    __syncthreads();
    const int ch = 64 * wave + 4 * li;
    double wacc[4][4][4], bsum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bsum[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) wacc[i][j][r] = 0.0;
    }
    const int g0 = blockIdx.x * a.gpw, g1 = min(a.groups, g0 + a.gpw);
    for (int g = g0; g < g1; ++g) {
        const size_t base = group_base(a, g);
        gf4 acc[4][4];
        zero_acc(acc);
#pragma unroll 4
        for (int ks = 0; ks < kTok / 4; ++ks) {
            const int k = 4 * ks + q;
            const size_t pix = token_pixel(a, base, k);
            const gf4 dg = ld4(a.dgated + pix * kC + ch), av = ld4(a.gb + pix * kC2 + ch);
            const gf4 mp = ld4(a.mixp1_in + pix * kC + ch), hv = ld4(a.hb + pix * kC2 + ch);
            const gf4 dm = dg * av;
            gf4 dh;
#pragma unroll
            for (int j = 0; j < 4; ++j) dh[j] = (dg[j] * mp[j]) * gelu_grad(hv[j]);
            st4(a.dhb + pix * kC2 + ch, dh);
            float w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = sW[k][16 * i + li];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], dm[j], acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t pix = token_pixel(a, base, 16 * i + 4 * q + r);
                st4(a.dcn + pix * kC + ch, gf4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]});
            }
        // dWt over channels 64 wave + 16 q + s: the A operand (m = p = 16 i + li) is dmix, the B operand (n = q' = 16 j + li) is cn
        zero_acc(acc);
        size_t pa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pa[i] = token_pixel(a, base, 16 * i + li);
        const int c0 = 64 * wave + 16 * q;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            gf4 am[4], bc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                am[i] = ld4(a.dgated + pa[i] * kC + c0 + 4 * s4) * ld4(a.gb + pa[i] * kC2 + c0 + 4 * s4);
                bc[i] = ld4(a.cn + pa[i] * kC + c0 + 4 * s4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    bsum[i] += (double)am[i][e];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[i][e], bc[j][e], acc[i][j], 0, 0, 0);
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) wacc[i][j][r] += (double)acc[i][j][r];
    }
    double *out = a.part + ((size_t)blockIdx.x * (kC / 64) + wave) * kMixPart;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(16 * i + 4 * q + r) * kTok + 16 * j + li] = wacc[i][j][r];
        double v = bsum[i];                 // token 16 i + li over this lane's sixteen channels: add the four quarters
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (q == 0) out[kTok * kTok + 16 * i + li] = v;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// check_sizes, and in front of its pixel count the 8 x 8 grid and the 8 x 8 blocks (N is a multiple of 64 behind that rule)
int check_gmlp_sizes(int B, int Hc, int Wc) {
    if (B < 1 || B > kMaxPairs || Hc < 1 || Wc < 1) return BALF_ERR_ARG;
    if (Hc % 8 || Wc % 8) return BALF_ERR_SHAPE;
    return check_sizes(B, Hc, Wc);
}

MixArgs mix_args(const Layout &l, bool grid) {
    MixArgs m{};
    const int fh = l.Hc / 8, fw = l.Wc / 8;
    m.groups = l.groups; m.gpw = l.gpw;
    m.per_img = fh * fw; m.fw = fw; m.HW = l.Hc * l.Wc;
    if (grid) { m.by = l.Wc; m.bx = 1; m.sy = fh * l.Wc; m.sx = fw; }     // group = a place inside the region, token = the region
    else { m.by = 8 * l.Wc; m.bx = 8; m.sy = l.Wc; m.sx = 1; }            // group = a block, token = a place inside the block
    return m;
}

int check_call(const float *const *params, const void *const *others, int n_others, const void *const *aligned, int n_aligned) {
    if (!params) return BALF_ERR_ARG;
    for (int i = 0; i < kParams; ++i)
        if (!params[i] || misaligned(params[i], 15)) return BALF_ERR_ARG;
    for (int i = 0; i < n_others; ++i)
        if (!others[i]) return BALF_ERR_ARG;
    for (int i = 0; i < n_aligned; ++i)
        if (misaligned(aligned[i], 15)) return BALF_ERR_ARG;
    return BALF_OK;
}

template <int kC>
size_t layout_bytes(int B, int Hc, int Wc, bool saved) {
    size_t sv = 0, ws = 0;
    make_layout<kC>(B, Hc, Wc, nullptr, nullptr, &sv, &ws);
    return saved ? sv : ws;
}

template <int kC>
int gmlp_forward(const float *x0_dev, const float *const *params, int B, int Hc, int Wc, float *y_dev, void *saved_dev,
                 void *workspace_dev, size_t workspace_bytes, void *stream) {
    constexpr int kC2 = 2 * kC;
    const void *ptrs[] = {x0_dev, y_dev, saved_dev, workspace_dev};
    BALF_TRY(check_call(params, ptrs, 4, ptrs, 4));
    BALF_TRY(check_gmlp_sizes(B, Hc, Wc));
    if (workspace_bytes < layout_bytes<kC>(B, Hc, Wc, false)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout l = make_layout<kC>(B, Hc, Wc, static_cast<char *>(saved_dev), static_cast<char *>(workspace_dev), nullptr, nullptr);
    const int N = l.px.N;
    const float *const *P = params;

    BALF_TRY(ln_forward<kC>(x0_dev, kC, P[0], P[1], N, l.n0, l.stat0, st));
    BALF_TRY((pixel_gemm<EPI_BIAS_N_GELU, false>(l.n0, kC, kC, P[2], kC2, N, l.g0, kC2, P[3], l.h0, st)));      // (u, v) = gelu(n0 W1^T + b1)
    for (int k = 0; k < 2; ++k) {
        const Branch &b = l.br[k];
        const float *const *Q = P + 4 + kBranchParams * k;
        const float *z = l.g0 + kC * k;                                                              // u or v, row stride 512
        BALF_TRY(ln_forward<kC>(z, kC2, Q[0], Q[1], N, b.nb, b.statb, st));
        BALF_TRY((pixel_gemm<EPI_BIAS_N_GELU, false>(b.nb, kC, kC, Q[2], kC2, N, b.gb, kC2, Q[3], b.hb, st)));   // (a, c)
        BALF_TRY(ln_forward<kC>(b.gb + kC, kC2, Q[4], Q[5], N, b.cn, b.statg, st));
        MixArgs m = mix_args(l, k == 0);
        m.wt = Q[6]; m.bt = Q[7]; m.cn = b.cn; m.gb = b.gb; m.mixp1 = b.mixp1; m.gated = b.gated;
        mix_fwd_kernel<kC><<<l.groups, kC, 0, st>>>(m);
        BALF_LAUNCH_CHECK();
        BALF_TRY((pixel_gemm<EPI_BIAS_N_ADD, false>(b.gated, kC, kC, Q[8], kC, N, l.cat + kC * k, kC2, Q[9], z, st)));   // z' = z + gated Wb2^T + bb2
    }
    return pixel_gemm<EPI_BIAS_N_ADD, false>(l.cat, kC2, kC2, P[24], kC, N, y_dev, kC, P[25], x0_dev, st);      // y = cat W2^T + b2 + x0
}

template <int kC>
int gmlp_backward(const float *dy_dev, const float *x0_dev, const float *const *params, const void *saved_dev, int B, int Hc, int Wc,
                  float *const *grads, float *dx0_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    constexpr int kC2 = 2 * kC;
    const void *ptrs[] = {dy_dev, x0_dev, saved_dev, workspace_dev, dx0_dev};
    BALF_TRY(check_call(params, ptrs, 4, ptrs, 5));
    if (!grads) return BALF_ERR_ARG;
    for (int i = 0; i < kParams; ++i)
        if (!grads[i]) return BALF_ERR_ARG;
    BALF_TRY(check_gmlp_sizes(B, Hc, Wc));
    if (workspace_bytes < layout_bytes<kC>(B, Hc, Wc, false)) return BALF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout l = make_layout<kC>(B, Hc, Wc, static_cast<char *>(const_cast<void *>(saved_dev)), static_cast<char *>(workspace_dev),
                                 nullptr, nullptr);
    const int N = l.px.N;
    const float *const *P = params;
    float *const *G = grads;
    double *part0 = l.col_part, *part1 = l.col_part + (size_t)l.px.PC * kC2;
    LnBwdArgs n{};                                                                                   // what the five LayerNorms share
    n.part_g = part0; n.part_b = part1;

    // y = cat W2^T + b2 + x0:  db2 = sum dy,  dW2 = dy^T cat,  dcat = dy W2
    BALF_TRY(bias_grad(dy_dev, kC, kC, l.px, part0, G[25], st));
    BALF_TRY(weight_grad(dy_dev, kC, kC, l.cat, kC2, kC2, l.px, l.slab, G[24], st));
    BALF_TRY((pixel_gemm<EPI_STORE, true>(dy_dev, kC, kC, P[24], kC2, N, l.dcat, kC2, nullptr, nullptr, st)));
    for (int k = 0; k < 2; ++k) {
        const Branch &b = l.br[k];
        const float *const *Q = P + 4 + kBranchParams * k;
        float *const *D = G + 4 + kBranchParams * k;
        const float *dzo = l.dcat + kC * k;                                                          // the gradient at z', row stride 512
        // z' = z + gated Wb2^T + bb2
        BALF_TRY(bias_grad(dzo, kC2, kC, l.px, part0, D[9], st));
        BALF_TRY(weight_grad(dzo, kC2, kC, b.gated, kC, kC, l.px, l.slab, D[8], st));
        float *dgated = l.t0, *dcn = l.t1;
        BALF_TRY((pixel_gemm<EPI_STORE, true>(dzo, kC2, kC, Q[8], kC, N, dgated, kC, nullptr, nullptr, st)));
        // the gate and the token mix: dhb (a's half), dcn, dWt, dbt
        MixArgs m = mix_args(l, k == 0);
        m.wt = Q[6]; m.cn = b.cn; m.gb = b.gb; m.dgated = dgated; m.hb = b.hb; m.mixp1_in = b.mixp1; m.dhb = l.dhb; m.dcn = dcn;
        m.part = l.mix_part;
        mix_bwd_kernel<kC><<<l.PW, kC, 0, st>>>(m);
        BALF_LAUNCH_CHECK();
        partial_sum_kernel<<<kTok * kTok / 4, 256, 0, st>>>(l.mix_part, kTok * kTok, (kC / 64) * l.PW, 1, (size_t)kMixPart, D[6], nullptr);
        BALF_LAUNCH_CHECK();
        partial_sum_kernel<<<kTok / 4, 256, 0, st>>>(l.mix_part + kTok * kTok, kTok, (kC / 64) * l.PW, 1, (size_t)kMixPart, D[7], nullptr);
        BALF_LAUNCH_CHECK();
        // the gating LayerNorm on c: dhb (c's half) = LN'(dcn) * gelu'(hb)
        n.dn = dcn; n.stat = b.statg; n.ln_g = Q[4];
        n.x = b.gb + kC; n.xs = kC2; n.h = b.hb + kC; n.hs = kC2; n.out = l.dhb + kC; n.os = kC2;
        BALF_TRY((ln_backward<kC, LN_DX_GELU>(n, l.px, D[4], D[5], st)));
        // hb = nb Wb1^T + bb1
        BALF_TRY(bias_grad(l.dhb, kC2, kC2, l.px, part0, D[3], st));
        BALF_TRY(weight_grad(l.dhb, kC2, kC2, b.nb, kC, kC, l.px, l.slab, D[2], st));
        float *dnb = l.t0;                                                                           // dgated is spent
        BALF_TRY((pixel_gemm<EPI_STORE, true>(l.dhb, kC2, kC2, Q[2], kC, N, dnb, kC, nullptr, nullptr, st)));
        // the branch's LayerNorm on z and its shortcut: dh0 (this half) = (dzo + LN'(dnb)) * gelu'(h0)
        n.dn = dnb; n.stat = b.statb; n.ln_g = Q[0];
        n.x = l.g0 + kC * k; n.xs = kC2; n.g = dzo; n.gs = kC2; n.h = l.h0 + kC * k; n.hs = kC2; n.out = l.dh0 + kC * k; n.os = kC2;
        BALF_TRY((ln_backward<kC, LN_DX_ADD_GELU>(n, l.px, D[0], D[1], st)));
    }
    // h0 = n0 W1^T + b1
    BALF_TRY(bias_grad(l.dh0, kC2, kC2, l.px, part0, G[3], st));
    BALF_TRY(weight_grad(l.dh0, kC2, kC2, l.n0, kC, kC, l.px, l.slab, G[2], st));
    float *dn0 = l.t0;
    BALF_TRY((pixel_gemm<EPI_STORE, true>(l.dh0, kC2, kC2, P[2], kC, N, dn0, kC, nullptr, nullptr, st)));
    // the layer's LayerNorm and its shortcut: dx0 = dy + LN'(dn0)
    n.dn = dn0; n.stat = l.stat0; n.ln_g = P[0];
    n.x = x0_dev; n.xs = kC; n.g = dy_dev; n.gs = kC; n.h = nullptr; n.out = dx0_dev; n.os = kC;
    n.vec_g = true; n.vec_out = true;
    return dx0_dev ? ln_backward<kC, LN_DX_ADD>(n, l.px, G[0], G[1], st) : ln_backward<kC, LN_DX_NONE>(n, l.px, G[0], G[1], st);
}

}  // namespace

// the unit's two sizes for balf_train_unit_sizes (train_sizes.hip): the code of the size check, and the outputs only with BALF_OK
int gmlp_train_sizes(int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    BALF_TRY(check_gmlp_sizes(B, Hc, Wc));
    *workspace_bytes = C == 128 ? layout_bytes<128>(B, Hc, Wc, false) : layout_bytes<256>(B, Hc, Wc, false);
    *saved_bytes = C == 128 ? layout_bytes<128>(B, Hc, Wc, true) : layout_bytes<256>(B, Hc, Wc, true);
    return BALF_OK;
}

}  // namespace balf

using namespace balf;

extern "C" size_t balf_gmlp_train_workspace_bytes(int B, int Hc, int Wc) {
    return check_gmlp_sizes(B, Hc, Wc) == BALF_OK ? layout_bytes<256>(B, Hc, Wc, false) : 0;
}

extern "C" size_t balf_gmlp_train_saved_bytes(int B, int Hc, int Wc) {
    return check_gmlp_sizes(B, Hc, Wc) == BALF_OK ? layout_bytes<256>(B, Hc, Wc, true) : 0;
}

extern "C" int balf_gmlp_train_forward_c(const float *x0_dev, const float *const *params, int B, int Hc, int Wc, int C, float *y_dev,
                                         void *saved_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    return (C == 128 ? gmlp_forward<128> : gmlp_forward<256>)(x0_dev, params, B, Hc, Wc, y_dev, saved_dev, workspace_dev, workspace_bytes,
                                                              stream);
}

extern "C" int balf_gmlp_train_backward_c(const float *dy_dev, const float *x0_dev, const float *const *params, const void *saved_dev,
                                          int B, int Hc, int Wc, int C, float *const *grads, float *dx0_dev, void *workspace_dev,
                                          size_t workspace_bytes, void *stream) {
    if (C != 128 && C != 256) return BALF_ERR_SHAPE;
    return (C == 128 ? gmlp_backward<128> : gmlp_backward<256>)(dy_dev, x0_dev, params, saved_dev, B, Hc, Wc, grads, dx0_dev, workspace_dev,
                                                                workspace_bytes, stream);
}

extern "C" int balf_gmlp_train_forward(const float *x0_dev, const float *const *params, int B, int Hc, int Wc, float *y_dev,
                                       void *saved_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return balf_gmlp_train_forward_c(x0_dev, params, B, Hc, Wc, 256, y_dev, saved_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int balf_gmlp_train_backward(const float *dy_dev, const float *x0_dev, const float *const *params, const void *saved_dev,
                                        int B, int Hc, int Wc, float *const *grads, float *dx0_dev, void *workspace_dev,
                                        size_t workspace_bytes, void *stream) {
    return balf_gmlp_train_backward_c(dy_dev, x0_dev, params, saved_dev, B, Hc, Wc, 256, grads, dx0_dev, workspace_dev, workspace_bytes,
                                      stream);
}
