// The shared pieces of the training kernels (head_train.hip, rcab_train.hip, gmlp_train.hip, linrelu_train.hip, and the x0
// recomputation of stage_view.hip):
//   * gemm_kernel: ONE LDS-tiled GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains, k ascending).  A workgroup of four waves
//     owns a 64 x 64 tile of C[m][n] = sum_k A(m,k) * B(k,n), a wave a 32 x 32 quarter (2 x 2 MFMA tiles); K goes through LDS in
//     steps of 16 with the next step's operands fetched into registers before the MFMAs of this one.  The operands are addressed
//     by (row stride, k stride); whatever lies outside M, Nn or the K range is never loaded and enters the tile as 0, and a
//     16-row MFMA tile wholly outside is skipped.  A weight gradient sums over the pixels: its K range is cut into S slices
//     (rows_per_slice(N)), slice s writes slab s of the workspace, and slab_sum_kernel adds the S slabs in float64 in slice order.
//   * the float64 sums over pixels: chain4_sum, the ONE spelling of a thread's sum over a block of rows (four chains, row r on
//     chain (r - r0) % 4), which col_sum_kernel (per-workgroup partials of the columns of a strided matrix, 256 columns per grid y)
//     and the RCAB's img_sum_kernel / dt_kernel call with their own terms, and partial_sum_kernel (a wave per output adds the
//     partials in one fixed order: lanes strided, then the butterfly).
//   * ld4 / st4, the 16-byte accesses of four consecutive channels, with the overloads that fall back to four 4-byte accesses.
//   * the host side: PixelSlices, the slice geometry of N pixels that every unit's Layout holds; check_sizes, the limits of
//     (B, Hc, Wc); and the launch helpers pixel_gemm / weight_grad / finish_cols / bias_grad, which fill a GemmArgs for the
//     products along the channels of pixel-major matrices and launch the column sums.  Every helper checks each of its launches
//     and returns BALF_OK or BALF_ERR_LAUNCH; a caller passes that on with BALF_TRY.
// An epilogue is a template value: a new one adds an instantiation and leaves the code of the others as it was.
#pragma once
#include "block_ops.h"

namespace balf {
namespace {

typedef float gf4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64, kTK = 16, kPitch = kTile + 4;
constexpr int kMaxSlices = 64;              // slabs of a weight gradient
constexpr int kTrainMaxN = 1 << 24;         // pixels: up to 2^32 elements in a [N,256] matrix, indexed in size_t

// pass on the status of a check or of a launch helper unless it is BALF_OK
#define BALF_TRY(call)                            \
    do {                                          \
        const int balf_try_rc = (call);           \
        if (balf_try_rc != BALF_OK)               \
            return balf_try_rc;                   \
    } while (0)

bool misaligned(const void *p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

// B images of Hc x Wc cells, N = B * Hc * Wc pixels: the limits of the head, and of the RCAB, whose output is the head's input
int check_sizes(int B, int Hc, int Wc) {
    if (B < 1 || B > kMaxPairs || Hc < 1 || Wc < 1) return BALF_ERR_ARG;
    const long n = (long)B * (long)Hc * (long)Wc;
    if (n > (long)kTrainMaxN) return BALF_ERR_SHAPE;
    if (n < 2) return BALF_ERR_ARG;         // one value per channel has no variance
    return BALF_OK;
}

__device__ __forceinline__ gf4 ld4(const float *p) { return *reinterpret_cast<const gf4 *>(p); }
__device__ __forceinline__ void st4(float *p, gf4 v) { *reinterpret_cast<gf4 *>(p) = v; }
// (vec, uniform: the array is 16-byte aligned; else four 4-byte accesses)
__device__ __forceinline__ gf4 ld4(const float *p, bool vec) { return vec ? ld4(p) : gf4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st4(float *p, gf4 v, bool vec) {
    if (vec) { st4(p, v); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = v[j];
}

// rows (pixels) per K slice of dW2 / dWd: 256, or the multiple of 256 that keeps the slices at kMaxSlices
int rows_per_slice(int N) {
    const int chunks = balf_ceil_div(N, 256);
    return 256 * balf_ceil_div(chunks, kMaxSlices);
}

// How the N pixels are cut: S slices of rows pixels for the K range of a weight gradient, PC workgroups of col_rows rows for the
// float64 column sums (64 rows per workgroup, or what keeps PC at 1024)
struct PixelSlices {
    int N, rows, S, col_rows, PC;
};

PixelSlices pixel_slices(int N) {
    PixelSlices p{};
    p.N = N;
    p.rows = rows_per_slice(N);
    p.S = balf_ceil_div(N, p.rows);
    p.col_rows = p.rows / 16 > 64 ? p.rows / 16 : 64;
    p.PC = balf_ceil_div(N, p.col_rows);
    return p;
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------------------
// EPI_BIAS_N: + bias[n];  EPI_BIAS_N_LRELU: + bias[n], then v > 0 ? v : 0.2 v;  EPI_LRELU_MASK: mask > 0 ? v : 0.2 v (the LeakyReLU's
// derivative from its OUTPUT: the output has the sign of the input, and 0.2 at 0 as torch);  EPI_BIAS_N_GELU: h = v + bias[n] is
// STORED at mask's place (the pre-activation, which the backward takes the derivative from) and C gets gelu(h), the exact erf
// form;  EPI_BIAS_N_ADD: (v + bias[n]) + mask, a shortcut laid out as C
enum { EPI_STORE = 0, EPI_BIAS_N_RELU = 1, EPI_BIAS_M = 2, EPI_RELU_MASK = 3, EPI_BIAS_N = 4, EPI_BIAS_N_LRELU = 5, EPI_LRELU_MASK = 6,
       EPI_BIAS_N_GELU = 7, EPI_BIAS_N_ADD = 8 };

// Phi(h), the normal distribution function, from erfc: no cancellation in the lower tail
__device__ __forceinline__ float normal_cdf(float h) { return 0.5f * erfcf(-0.70710678118654752f * h); }
// gelu(h) = h Phi(h) (nn.GELU(), approximate = 'none') and its derivative Phi(h) + h phi(h)
__device__ __forceinline__ float gelu_exact(float h) { return h * normal_cdf(h); }
__device__ __forceinline__ float gelu_grad(float h) {
    return fmaf(h, 0.39894228040143268f * expf(-0.5f * h * h), normal_cdf(h));
}

struct GemmArgs {
    const float *A, *B;
    size_t a_sm, a_sk, b_sn, b_sk;          // element (m, k) of A is A[m * a_sm + k * a_sk], (k, n) of B is B[n * b_sn + k * b_sk]
    int M, Nn, K, k_rows;                   // slice z sums k in [z * k_rows, min(K, (z + 1) * k_rows))
    float *C;
    size_t c_sm, c_sz;                      // C[z * c_sz + m * c_sm + n]
    const float *bias, *mask;               // the epilogue's: bias[n] or bias[m]; mask as C (EPI_RELU_MASK; written by EPI_BIAS_N_GELU)
};

// A_K / B_K: the operand is contiguous along k (else along m / n) -- decides which way the 256 threads walk its 64 x 16 tile
// PIX_N: the long dimension (pixels) is n and takes grid x
template <bool A_K, bool B_K, bool PIX_N, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
    __shared__ float sA[kTK][kPitch], sB[kTK][kPitch];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, li = lane & 15;
    const int m0 = (PIX_N ? blockIdx.y : blockIdx.x) * kTile, n0 = (PIX_N ? blockIdx.x : blockIdx.y) * kTile;
    const int kb = blockIdx.z * g.k_rows, ke = min(g.K, kb + g.k_rows);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    // (uniform per wave) the 16-wide MFMA tiles of this wave that hold a row / column inside the matrix
    const bool live_m[2] = {m0 + wm < g.M, m0 + wm + 16 < g.M}, live_n[2] = {n0 + wn < g.Nn, n0 + wn + 16 < g.Nn};

    int am[4], ak[4], bn[4], bk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = t + 256 * i;
        am[i] = A_K ? e >> 4 : e & 63;
        ak[i] = A_K ? e & 15 : e >> 6;
        bn[i] = B_K ? e >> 4 : e & 63;
        bk[i] = B_K ? e & 15 : e >> 6;
    }
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + am[i], ka = k0 + ak[i], n = n0 + bn[i], kk = k0 + bk[i];
            ra[i] = (m < g.M && ka < ke) ? g.A[(size_t)m * g.a_sm + (size_t)ka * g.a_sk] : 0.0f;
            rb[i] = (n < g.Nn && kk < ke) ? g.B[(size_t)n * g.b_sn + (size_t)kk * g.b_sk] : 0.0f;
        }
    };
    gf4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = gf4{0.0f, 0.0f, 0.0f, 0.0f};

    if (kb < ke) fetch(kb);
    for (int k0 = kb; k0 < ke; k0 += kTK) {
        __syncthreads();                                        // the MFMAs of the step before have read the tiles
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sA[ak[i]][am[i]] = ra[i];
            sB[bk[i]][bn[i]] = rb[i];
        }
        __syncthreads();
        if (k0 + kTK < ke) fetch(k0 + kTK);
#pragma unroll
        for (int ks = 0; ks < kTK / 4; ++ks) {
            const int k = 4 * ks + q;
            const float a0 = sA[k][wm + li], a1 = sA[k][wm + 16 + li], b0 = sB[k][wn + li], b1 = sB[k][wn + 16 + li];
            if (live_m[0] && live_n[0]) acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            if (live_m[0] && live_n[1]) acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            if (live_m[1] && live_n[0]) acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            if (live_m[1] && live_n[1]) acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // the accumulator holds column n = lane & 15 and rows 4 * (lane >> 4) + r of its 16 x 16 tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * q + r, n = n0 + wn + 16 * j + li;
                if (m >= g.M || n >= g.Nn) continue;
                const size_t at = (size_t)m * g.c_sm + (size_t)n;
                float v = acc[i][j][r];
                if (EPI == EPI_BIAS_N_RELU) v = fmaxf(v + g.bias[n], 0.0f);
                if (EPI == EPI_BIAS_M) v = v + g.bias[m];
                if (EPI == EPI_RELU_MASK) v = g.mask[at] > 0.0f ? v : 0.0f;
                if (EPI == EPI_BIAS_N) v = v + g.bias[n];
                if (EPI == EPI_BIAS_N_LRELU) { v = v + g.bias[n]; v = v > 0.0f ? v : 0.2f * v; }
                if (EPI == EPI_LRELU_MASK) v = g.mask[at] > 0.0f ? v : 0.2f * v;
                if (EPI == EPI_BIAS_N_GELU) { v = v + g.bias[n]; const_cast<float *>(g.mask)[at] = v; v = gelu_exact(v); }
                if (EPI == EPI_BIAS_N_ADD) v = (v + g.bias[n]) + g.mask[at];
                g.C[(size_t)blockIdx.z * g.c_sz + at] = v;
            }
}

template <bool A_K, bool B_K, bool PIX_N, int EPI>
void launch_gemm(const GemmArgs &g, hipStream_t st) {
    const int mt = balf_ceil_div(g.M, kTile), nt = balf_ceil_div(g.Nn, kTile), zs = balf_ceil_div(g.K, g.k_rows);
    const dim3 grid(PIX_N ? nt : mt, PIX_N ? mt : nt, zs);
    gemm_kernel<A_K, B_K, PIX_N, EPI><<<grid, 256, 0, st>>>(g);
}

// out[i] = fl32(sum over the S slabs, slab 0 first, in float64)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float *slab, int S, int count, float *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double s = 0.0;
    for (int z = 0; z < S; ++z) s += (double)slab[(size_t)z * count + i];
    out[i] = (float)s;
}

// ---- float64 sums over pixels ----------------------------------------------------------------------------------------------
// sum of P partials part[i * stride], to every lane of the wave: lanes strided over the partials, then the butterfly
__device__ __forceinline__ double wave_sum_strided(const double *part, int P, size_t stride) {
    double s = 0.0;
    for (int i = threadIdx.x & 63; i < P; i += 64) s += part[(size_t)i * stride];
    return wave_sum(s);
}

// one wave per output: out[c] = fl32(sum_p part[c * stride_c + p * stride_p]), out64[c] the float64 sum (either may be NULL)
__global__ __launch_bounds__(256) void partial_sum_kernel(const double *part, int count, int P, size_t stride_c, size_t stride_p,
                                                          float *out, double *out64) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= count) return;
    const double s = wave_sum_strided(part + (size_t)c * stride_c, P, stride_p);
    if ((threadIdx.x & 63) == 0) {
        if (out) out[c] = (float)s;
        if (out64) out64[c] = s;
    }
}

// where row r >= 0 of a matrix of row stride s begins, in elements: one 32 x 32 -> 64-bit product, which a row loop waits for
// before it can issue the row's load (a stride held in 64 bits costs three products and their sums)
__device__ __forceinline__ size_t row_at(int r, unsigned s) { return (size_t)(unsigned)r * s; }

// the float64 sum of term(r) over rows [r0, r1): row r goes to chain (r - r0) % 4, four rows (loads) in flight, and the chains are
// added as (s0 + s1) + (s2 + s3)
template <typename Term>
__device__ __forceinline__ double chain4_sum(int r0, int r1, Term term) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += term(r + i);
    }
    for (int i = 0; r < r1; ++r, ++i) s[i] += term(r);
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// float64 column sums of rows [blockIdx.x * rows, ...) of a matrix of row stride xs and cols columns (256 per grid y; 128: half a
// workgroup idles), a column per thread: part[block][column]
__global__ __launch_bounds__(256) void col_sum_kernel(const float *x, unsigned xs, int N, int rows, int cols, double *part) {
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows), c = blockIdx.y * 256 + threadIdx.x;
    if (c >= cols) return;
    part[(size_t)blockIdx.x * cols + c] = chain4_sum(r0, r1, [&](int r) { return (double)x[row_at(r, xs) + c]; });
}

// ---- the launches along the channels -----------------------------------------------------------------------------------------
// C[pixel][n] = epilogue(sum_k A[pixel * lda + k] * W(k, n)), n < Nn, k < K: TRANSPOSED = false reads W[n][k] (x W^T), true reads
// W[k][n] (x W)
template <int EPI, bool TRANSPOSED>
int pixel_gemm(const float *A, size_t lda, int K, const float *W, int Nn, int N, float *C, size_t ldc, const float *bias,
                const float *mask, hipStream_t st) {
    GemmArgs g{};
    g.A = A; g.a_sm = lda; g.a_sk = 1;
    g.B = W; g.b_sn = TRANSPOSED ? 1 : K; g.b_sk = TRANSPOSED ? Nn : 1;
    g.M = N; g.Nn = Nn; g.K = K; g.k_rows = K;
    g.C = C; g.c_sm = ldc; g.bias = bias; g.mask = mask;
    launch_gemm<true, !TRANSPOSED, false, EPI>(g, st);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// out[o][k] = fl32(sum_pixel D[pixel * ldd + o] * X[pixel * ldx + k]), o < M, k < Nn, in p.S slices of the pixels through slab
// [p.S][M * Nn], the slabs added in float64.  (A template only so that a unit that never calls it instantiates no GEMM for it.)
template <typename = void>
int weight_grad(const float *D, size_t ldd, int M, const float *X, size_t ldx, int Nn, const PixelSlices &p, float *slab, float *out,
                 hipStream_t st) {
    GemmArgs g{};
    g.A = D; g.a_sm = 1; g.a_sk = ldd;
    g.B = X; g.b_sn = 1; g.b_sk = ldx;
    g.M = M; g.Nn = Nn; g.K = p.N; g.k_rows = p.rows;
    g.C = slab; g.c_sm = Nn; g.c_sz = (size_t)M * Nn;
    launch_gemm<false, false, false, EPI_STORE>(g, st);
    BALF_LAUNCH_CHECK();
    slab_sum_kernel<<<M * Nn / 256, 256, 0, st>>>(slab, p.S, M * Nn, out);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// out[c] = fl32(sum over the P float64 partials part[p][c] of column c), c < cols
int finish_cols(const double *part, int cols, int P, float *out, hipStream_t st) {
    partial_sum_kernel<<<cols / 4, 256, 0, st>>>(part, cols, P, 1, (size_t)cols, out, nullptr);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

// a bias gradient: out[c] = fl32(sum over the p.N rows of x[row * xs + c]), c < cols (128, 256 or 512), through part [p.PC][cols]
int bias_grad(const float *x, unsigned xs, int cols, const PixelSlices &p, double *part, float *out, hipStream_t st) {
    col_sum_kernel<<<dim3(p.PC, balf_ceil_div(cols, 256)), 256, 0, st>>>(x, xs, p.N, p.col_rows, cols, part);
    BALF_LAUNCH_CHECK();
    return finish_cols(part, cols, p.PC, out, st);
}

}  // namespace
}  // namespace balf
