// The pieces of compute_repeatability (balf/benchmark_test/repeatability_tools.py:379-512) that the one-pair entry
// (balf_repeatability, repeat.hip) and the batched one (balf_repeatability_batch, repeat_batch.hip) share, so that the two
// compute the same bits: the circle overlaps of a pair of points, the descending stable radix sort of a candidate list and
// the greedy assignment walk over the sorted list.  All arithmetic is float64, like the reference's Python floats.
#pragma once
#include <hip/hip_runtime.h>

namespace balf {
namespace {

constexpr double kPi = 3.141592653589793;
constexpr double kEpsF64 = 2.220446049250313e-16;          // np.finfo(float).eps
constexpr int kMaxPoints = 65536;                          // visited bitmaps live in LDS
constexpr int kSortWaves = 16;

struct RepParams {
    double thr, eps, dist_match, radius, max_dist;
};

__device__ __forceinline__ double inter_area(double R, double r, double d) {
    if (d <= fabs(R - r)) { const double m = fmin(R, r); return kPi * (m * m); }
    if (d >= r + R) return 0.0;
    const double r2 = r * r, R2 = R * R, d2 = d * d;
    const double alpha = acos((d2 + r2 - R2) / (2 * d * r));
    const double beta = acos((d2 + R2 - r2) / (2 * d * R));
    return r2 * alpha + R2 * beta - 0.5 * (r2 * sin(2 * alpha) + R2 * sin(2 * beta));
}

__device__ __forceinline__ void pair_overlaps(double sx, double sy, double sr, double tx, double ty, double tr,
                                              const RepParams &p, double &single, double &multi, bool &possible) {
    const double dx = sx - tx, dy = sy - ty;
    const double dist = sqrt(dx * dx + dy * dy);
    possible = dist <= p.dist_match;
    single = 0.0; multi = 0.0;
    if (dist > p.max_dist) return;
    const double f = p.radius / (fmax(sr, tr) + kEpsF64);
    double I = inter_area(f * sr, f * tr, dist);
    double U = kPi * ((f * sr) * (f * sr)) + kPi * ((f * tr) * (f * tr)) - I + p.eps;
    multi = I / U;
    I = inter_area(p.radius, p.radius, dist);
    U = kPi * (p.radius * p.radius) + kPi * (p.radius * p.radius) - I + p.eps;
    single = I / U;
}

// Stable LSD radix sort of n (key, value) pairs, DESCENDING by the 64-bit key, 4 bits per pass, run by one workgroup of
// kSortWaves waves (every thread calls it; n is uniform).  Wave w owns the contiguous range [w * per, (w + 1) * per) of the
// input and walks it 64 elements at a time, so "input order" is (wave, row, lane) and a pass keeps it among equal digits: per
// row the lane's rank among the lanes with its digit comes from a ballot, per wave the digit counts go through a [digit][wave]
// table in LDS (hist) whose exclusive scan (digit-major) gives every wave its output cursor per digit.  Passes whose digit is
// the same for all keys are skipped (overlaps lie in [1 - overlap_err, 1]: the sign, exponent and leading mantissa digits
// agree), so the 16 possible passes are ~11 in practice.  The pairs ping-pong between (k0, v0) and (k1, v1); the result
// always ends in (k1, v1).  The sorted order is unique (stable sort), so it does not depend on the wave split.
__device__ __forceinline__ void rep_sort_pairs(unsigned long long *k0, unsigned *v0, unsigned long long *k1, unsigned *v1,
                                               int n, int (*hist)[kSortWaves], int *uniform_digit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = ((n + kSortWaves - 1) / kSortWaves + 63) / 64 * 64;
    const int lo = wave * per < n ? wave * per : n, hi = lo + per < n ? lo + per : n;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long *kin = k0, *kout = k1;
    unsigned *vin = v0, *vout = v1;
    for (int shift = 0; shift < 64; shift += 4) {
        int cnt[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) cnt[d] = 0;
        for (int e0 = lo; e0 < hi; e0 += 64) {
            const int e = e0 + lane;
            const int dig = e < hi ? 15 - (int)((kin[e] >> shift) & 15ull) : -1;       // descending: largest digit first
#pragma unroll
            for (int d = 0; d < 16; ++d) cnt[d] += __popcll(__ballot(dig == d));
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < 16; ++d) hist[d][wave] = cnt[d];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int run = 0, uni = -1;
            for (int d = 0; d < 16; ++d) {
                int tot = 0;
                for (int w = 0; w < kSortWaves; ++w) { const int c = hist[d][w]; hist[d][w] = run; run += c; tot += c; }
                if (tot == n) uni = d;
            }
            *uniform_digit = uni;
        }
        __syncthreads();
        const bool skip = *uniform_digit >= 0;                   // every key has this digit: the pass would be the identity
        if (!skip) {
            int cur[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) cur[d] = hist[d][wave];
            for (int e0 = lo; e0 < hi; e0 += 64) {
                const int e = e0 + lane;
                unsigned long long k = 0; unsigned v = 0;
                if (e < hi) { k = kin[e]; v = vin[e]; }
                const int dig = e < hi ? 15 - (int)((k >> shift) & 15ull) : -1;
                int dst = 0;
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const unsigned long long b = __ballot(dig == d);
                    if (dig == d) dst = cur[d] + __popcll(b & below);
                    cur[d] += __popcll(b);
                }
                if (e < hi) { kout[dst] = k; vout[dst] = v; }
            }
        }
        __syncthreads();                                         // the pass's writes are visible to the whole workgroup; hist is free
        if (!skip) {
            unsigned long long *tk = kin; kin = kout; kout = tk;
            unsigned *tv = vin; vin = vout; vout = tv;
        }
    }
    if (kin != k1)                                               // (uniform) the sorted pairs sit in (k0, v0): copy
        for (int e = threadIdx.x; e < n; e += kSortWaves * 64) { k1[e] = kin[e]; v1[e] = vin[e]; }
}

// Greedy assignment over the n_edges sorted candidates (key = overlap bits, value = flat index y * nd + x), run by ONE wave
// (every lane calls it).  The wave walks the list 64 at a time; a candidate is taken when neither its destination x nor its
// source y is visited yet (bitmaps in LDS, the first words_x / words_y words are cleared here); the error sum is accumulated
// in the reference's order.  Lane 0 writes the assigned pairs (x, y) to corr while found < cap (cap = 0: none).  found and err
// come out the same in every lane.
__device__ __forceinline__ void rep_greedy_walk(const unsigned long long *keys, const unsigned *vals, int n_edges, int nd,
                                                unsigned *vis_x, unsigned *vis_y, int words_x, int words_y, int *corr,
                                                int cap, int &found_out, double &err_out) {
    const int lane = threadIdx.x;
    for (int k = lane; k < words_x; k += 64) vis_x[k] = 0u;
    for (int k = lane; k < words_y; k += 64) vis_y[k] = 0u;
    __syncthreads();
    int found = 0;
    double err = 0.0;
    for (int base = 0; base < n_edges; base += 64) {
        const int e = base + lane;
        unsigned idx = 0; double w = 0.0;
        if (e < n_edges) { idx = vals[e]; w = __longlong_as_double((long long)keys[e]); }
        const int yi = (int)(idx / (unsigned)nd), xj = (int)(idx % (unsigned)nd);
        const int lim = n_edges - base < 64 ? n_edges - base : 64;
        for (int l = 0; l < lim; ++l) {
            const int y = __shfl(yi, l), x = __shfl(xj, l);
            const double wl = __shfl(w, l);
            const bool taken = ((vis_x[x >> 5] >> (x & 31)) & 1u) || ((vis_y[y >> 5] >> (y & 31)) & 1u);
            if (!taken) {
                if (lane == 0) {
                    vis_x[x >> 5] |= 1u << (x & 31);
                    vis_y[y >> 5] |= 1u << (y & 31);
                    if (found < cap) { corr[2 * found] = x; corr[2 * found + 1] = y; }
                }
                found += 1;
                err += 1.0 - wl;
            }
            __syncthreads();        // single wave: orders lane 0's LDS update before the next read
        }
    }
    found_out = found;
    err_out = err;
}

}  // namespace
}  // namespace balf
