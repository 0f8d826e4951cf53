// balf_adam_step / balf_sgd_step (include/balf_hip.h): one optimiser step over up to BALF_OPTIM_MAX_TENSORS float32 tensors in ONE
// launch.  The multi-tensor-apply scheme: the device pointers, the element counts and the first-chunk prefix of every
// tensor that takes part travel in the kernel's argument block BY VALUE (2.8 KB for Adam at 64 tensors), so there is no device table,
// no upload and no workspace.
//
//   * workgroup b owns chunk b: kChunk consecutive elements of ONE tensor.  Its tensor is t = #{i : first[i] <= b} - 1, counted over
//     all 64 prefix entries with constant indices (entries past the last tensor hold INT_MAX): scalar loads and scalar compares, no
//     loop, uniform per workgroup.  Only the pointers of tensor t are then fetched with a (uniform) dynamic index.
//   * 16-byte accesses where every pointer of the tensor is 16-byte aligned (kChunk is a multiple of 4, so the chunk start is
//     aligned as the tensor is); 4-byte accesses otherwise, and for the up to three elements behind the last full quad.
//   * adam_elem / sgd_elem are the ONLY arithmetic, shared by both paths, compiled without contraction (the compiler forms no FMA;
//     the three of adam_elem are written out), with the correctly rounded division and square root that hipcc emits by default: an
//     element's result bits depend on its own inputs and the hyper-parameters alone -- not on alignment, on the position in a
//     tensor or on how the data is cut into tensors.
#include "common.h"

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace balf {
namespace {

constexpr int kMaxT = BALF_OPTIM_MAX_TENSORS;
constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 2;                                  // 16-byte accesses per thread, stream and chunk
constexpr int kChunk = kThreads * 4 * kQuadsPerThread;              // 2048 elements per workgroup
static_assert(kChunk % 4 == 0, "a chunk start keeps the tensor's 16-byte alignment");

typedef float f4 __attribute__((ext_vector_type(4)));

struct AdamHyper {
    float b1, omb1, b2, omb2, wd, step_size, sqrt_bc2, eps;         // omb = 1 - beta; step_size = lr / bc1
};

struct AdamArgs {
    float *p[kMaxT];
    const float *g[kMaxT];
    float *m[kMaxT];
    float *v[kMaxT];
    long long numel[kMaxT];
    int first[kMaxT];                                               // first chunk of tensor i; INT_MAX past the last tensor
    AdamHyper h;
};

struct SgdArgs {
    float *p[kMaxT];
    const float *g[kMaxT];
    long long numel[kMaxT];
    int first[kMaxT];
    float lr;
};

static_assert(sizeof(AdamArgs) <= 4096 && sizeof(SgdArgs) <= 4096, "the argument block of a kernel holds 4 KB");

// torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay), in this order.  The three sums of a product are explicit
// FMAs, one rounding each: with the hyper-parameters narrowed to float (1 - b2 = 0.001 is 0.8 u off) a separately rounded product
// would take v' to 8.5 u in the worst case, past the 6 u of its bound; with them it is 5.6 u.
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamHyper &h) {
    const float gp = h.wd != 0.0f ? fmaf(h.wd, p, g) : g;
    m = fmaf(h.omb1, gp, h.b1 * m);
    v = fmaf(h.omb2, gp * gp, h.b2 * v);
    const float den = sqrtf(v) / h.sqrt_bc2 + h.eps;
    p = p - (h.step_size * m) / den;
}

__device__ __forceinline__ void sgd_elem(float &p, float g, float lr) { p = p - lr * g; }

// the tensor of chunk b: the number of prefix entries <= b, minus one (first[0] = 0)
__device__ __forceinline__ int tensor_of(const int (&first)[kMaxT], int b) {
    int t = -1;
#pragma unroll
    for (int i = 0; i < kMaxT; ++i) t += first[i] <= b ? 1 : 0;
    return t;
}

__device__ __forceinline__ bool aligned16(const void *a, const void *b, const void *c, const void *d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

__global__ __launch_bounds__(kThreads) void adam_kernel(const AdamArgs a) {
    const int b = blockIdx.x;
    const int t = tensor_of(a.first, b);
    const size_t base = (size_t)(b - a.first[t]) * kChunk;
    const long long left = a.numel[t] - (long long)base;             // >= 1: the host launched ceil(numel / kChunk) chunks
    const int cnt = left < kChunk ? (int)left : kChunk;
    float *__restrict__ p = a.p[t] + base;
    const float *__restrict__ g = a.g[t] + base;
    float *__restrict__ m = a.m[t] + base;
    float *__restrict__ v = a.v[t] + base;
    const AdamHyper h = a.h;
    if (aligned16(p, g, m, v)) {
        const int quads = cnt >> 2;
        f4 pv[kQuadsPerThread], gv[kQuadsPerThread], mv[kQuadsPerThread], vv[kQuadsPerThread];
#pragma unroll
        for (int k = 0; k < kQuadsPerThread; ++k) {
            const int q = k * kThreads + threadIdx.x;
            if (q < quads) {
                pv[k] = reinterpret_cast<const f4 *>(p)[q];
                gv[k] = reinterpret_cast<const f4 *>(g)[q];
                mv[k] = reinterpret_cast<const f4 *>(m)[q];
                vv[k] = reinterpret_cast<const f4 *>(v)[q];
            }
        }
#pragma unroll
        for (int k = 0; k < kQuadsPerThread; ++k) {
            const int q = k * kThreads + threadIdx.x;
            if (q < quads) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float pe = pv[k][i], me = mv[k][i], ve = vv[k][i];
                    adam_elem(pe, gv[k][i], me, ve, h);
                    pv[k][i] = pe; mv[k][i] = me; vv[k][i] = ve;
                }
                reinterpret_cast<f4 *>(p)[q] = pv[k];
                reinterpret_cast<f4 *>(m)[q] = mv[k];
                reinterpret_cast<f4 *>(v)[q] = vv[k];
            }
        }
        const int e = 4 * quads + threadIdx.x;                       // the up to three elements behind the last full quad
        if (e < cnt) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_elem(pe, g[e], me, ve, h);
            p[e] = pe; m[e] = me; v[e] = ve;
        }
    } else {
        for (int e = threadIdx.x; e < cnt; e += kThreads) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_elem(pe, g[e], me, ve, h);
            p[e] = pe; m[e] = me; v[e] = ve;
        }
    }
}

__global__ __launch_bounds__(kThreads) void sgd_kernel(const SgdArgs a) {
    const int b = blockIdx.x;
    const int t = tensor_of(a.first, b);
    const size_t base = (size_t)(b - a.first[t]) * kChunk;
    const long long left = a.numel[t] - (long long)base;
    const int cnt = left < kChunk ? (int)left : kChunk;
    float *__restrict__ p = a.p[t] + base;
    const float *__restrict__ g = a.g[t] + base;
    const float lr = a.lr;
    if (aligned16(p, g, nullptr, nullptr)) {
        const int quads = cnt >> 2;
        f4 pv[kQuadsPerThread], gv[kQuadsPerThread];
#pragma unroll
        for (int k = 0; k < kQuadsPerThread; ++k) {
            const int q = k * kThreads + threadIdx.x;
            if (q < quads) {
                pv[k] = reinterpret_cast<const f4 *>(p)[q];
                gv[k] = reinterpret_cast<const f4 *>(g)[q];
            }
        }
#pragma unroll
        for (int k = 0; k < kQuadsPerThread; ++k) {
            const int q = k * kThreads + threadIdx.x;
            if (q < quads) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float pe = pv[k][i];
                    sgd_elem(pe, gv[k][i], lr);
                    pv[k][i] = pe;
                }
                reinterpret_cast<f4 *>(p)[q] = pv[k];
            }
        }
        const int e = 4 * quads + threadIdx.x;
        if (e < cnt) {
            float pe = p[e];
            sgd_elem(pe, g[e], lr);
            p[e] = pe;
        }
    } else {
        for (int e = threadIdx.x; e < cnt; e += kThreads) {
            float pe = p[e];
            sgd_elem(pe, g[e], lr);
            p[e] = pe;
        }
    }
}

bool misaligned4(const void *p) { return ((uintptr_t)p & 3) != 0; }
bool bad_scale(double x) { return !(x >= 0.0) || !std::isfinite(x); }      // negative, NaN or infinite
bool bad_beta(double b) { return !(b >= 0.0 && b < 1.0); }

// The checks both entry points share, in the header's order.  `m`, `v`: NULL arrays for SGD.
int check_tensors(int n, float *const *p, const float *const *g, float *const *m, float *const *v, bool adam, const int64_t *numel) {
    if (n < 1 || n > kMaxT || !p || !g || !numel || (adam && (!m || !v))) return BALF_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return BALF_ERR_ARG;
        if (numel[i] > 0 && (!p[i] || (adam && (!m[i] || !v[i])))) return BALF_ERR_ARG;
        if (misaligned4(p[i]) || misaligned4(g[i]) || (adam && (misaligned4(m[i]) || misaligned4(v[i])))) return BALF_ERR_ARG;
    }
    return BALF_OK;
}

// The tensors that take part (a gradient and at least one element), packed to the front of the argument block with their
// first-chunk prefix -> the number of chunks (0: nothing to do), or -1 when that exceeds 2^31 - 1.
template <class Args, class Put>
long long pack(int n, const float *const *g, const int64_t *numel, Args &a, Put put) {
    long long chunks = 0;
    int k = 0;
    for (int i = 0; i < n; ++i) {
        if (!g[i] || numel[i] == 0) continue;
        put(k, i);
        a.numel[k] = numel[i];
        a.first[k] = (int)chunks;
        chunks += (numel[i] + kChunk - 1) / kChunk;
        if (chunks > (long long)INT_MAX) return -1;
        ++k;
    }
    for (; k < kMaxT; ++k) a.first[k] = INT_MAX;
    return chunks;
}

}  // namespace
}  // namespace balf

using namespace balf;

extern "C" int balf_optim_chunk_elems(void) { return kChunk; }

extern "C" int balf_adam_step(int n, float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel,
                              double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream) {
    const int rc = check_tensors(n, p, g, m, v, true, numel);
    if (rc != BALF_OK) return rc;
    if (bad_scale(lr) || bad_scale(eps) || bad_scale(weight_decay) || bad_beta(beta1) || bad_beta(beta2) || step < 1) return BALF_ERR_ARG;
    AdamArgs a{};
    const long long chunks = pack(n, g, numel, a, [&](int k, int i) { a.p[k] = p[i]; a.g[k] = g[i]; a.m[k] = m[i]; a.v[k] = v[i]; });
    if (chunks < 0) return BALF_ERR_SHAPE;
    if (chunks == 0) return BALF_OK;
    // the bias corrections in double, as torch computes them on the host; the kernel gets floats
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    a.h.b1 = (float)beta1; a.h.omb1 = (float)(1.0 - beta1);
    a.h.b2 = (float)beta2; a.h.omb2 = (float)(1.0 - beta2);
    a.h.wd = (float)weight_decay;
    a.h.step_size = (float)(lr / bc1);
    a.h.sqrt_bc2 = (float)std::sqrt(bc2);
    a.h.eps = (float)eps;
    adam_kernel<<<(unsigned)chunks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

extern "C" int balf_sgd_step(int n, float *const *p, const float *const *g, const int64_t *numel, double lr, void *stream) {
    const int rc = check_tensors(n, p, g, nullptr, nullptr, false, numel);
    if (rc != BALF_OK) return rc;
    if (bad_scale(lr)) return BALF_ERR_ARG;
    SgdArgs a{};
    const long long chunks = pack(n, g, numel, a, [&](int k, int i) { a.p[k] = p[i]; a.g[k] = g[i]; });
    if (chunks < 0) return BALF_ERR_SHAPE;
    if (chunks == 0) return BALF_OK;
    a.lr = (float)lr;
    sgd_kernel<<<(unsigned)chunks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
