// Workgroup-level building blocks of the point kernels (nms_topk.hip, nms_fast.hip, multiscale.hip, repeat.hip,
// repeat_batch.hip, val_points.hip, resize_repeat.hip, match_eval.hip, and the pair filter of common_points.h that
// repeat_batch.hip and match_eval.hip share): ONE definition each of the select, scan, compaction, sort and
// reduction these kernels are assembled from, so that a barrier or a tie rule is fixed in one place.
// Every device function below that takes LDS is called by ALL threads of the workgroup (THREADS of them, a multiple of 64, x
// only), with the same arguments where a comment says "uniform".  The LDS is the caller's: nothing here declares __shared__,
// so a kernel that must keep zero static LDS keeps it.  Each function frees its own scratch with the barriers its comment
// lists, so it may be called again on the same LDS at once.
// Device building blocks (the host shares next_pow2 and kMaxPairs); the host's own helpers are in common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"

namespace balf {
namespace {

constexpr int kMaxPairs = 65535;            // pairs per batched call: the pair index is a grid y / z dimension

__host__ __device__ __forceinline__ int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- wave level (64 lanes, all active) ----------------------------------------------------------------------------------------
// (summed in the type of the argument: a bool or a comparison would be summed as such, hence the list)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_same<T, int>::value || std::is_same<T, unsigned>::value || std::is_same<T, float>::value ||
                      std::is_same<T, double>::value, "wave_sum: int, unsigned, float or double");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// a count written by an earlier kernel, read at element `at` and clamped to [0, n_max]
__device__ __forceinline__ int clamp_count(const int *c, long at, int n_max) {
    const int v = c[at];
    return v < 0 ? 0 : (v > n_max ? n_max : v);
}

// ---- workgroup level ----------------------------------------------------------------------------------------------------------
// Sum of v over the workgroup, returned to every thread.  Two barriers: before s_red is written (frees it), after.
// (int counts, and the float64 sums of detector_loss.hip: one fixed order, butterfly in the wave, then wave 0 upwards)
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T *s_red /*[THREADS / 64]*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) t += s_red[w];
    return t;
}

// One chunk (THREADS consecutive elements, element = thread) of a chunked exclusive scan of N independent sequences: v[c] is
// this thread's element of sequence c (0 past the end), excl[c] comes back as the sum of everything before it, in this chunk
// and in the earlier ones.  s_base[c] carries the running total from chunk to chunk: the caller zeroes it and passes a barrier
// before the first chunk, and reads the grand totals from it after the last.  Three barriers: after the per-wave sums are in
// s_wsum, before the last thread stores the new base (everyone has read the old one), and after that store.
template <typename T, int N, int THREADS>
__device__ __forceinline__ void block_scan_chunk(const T (&v)[N], T (&excl)[N], T (*s_wsum)[THREADS / 64], T *s_base /*[N]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        incl[c] = wave_incl_scan(v[c]);
        if (lane == 63) s_wsum[c][wave] = incl[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T before = s_base[c];
        for (int w = 0; w < wave; ++w) before += s_wsum[c][w];
        incl[c] += before;
        excl[c] = incl[c] - v[c];
    }
    __syncthreads();
    if (threadIdx.x == THREADS - 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) s_base[c] = incl[c];
    }
    __syncthreads();
}

// One chunk of an ordered (stable) compaction: the output slot of this thread's element if it is kept, counting the kept
// elements of lower threads in this chunk and `base` of the earlier chunks; base (a register, uniform) is advanced by the
// chunk's count.  Two barriers: one before s_wcnt is written (frees it), one after.
template <int THREADS>
__device__ __forceinline__ int compact_slot(bool keep, int *s_wcnt /*[THREADS / 64]*/, int &base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    __syncthreads();
    if (lane == 0) s_wcnt[wave] = __popcll(b);
    __syncthreads();
    int before = base, chunk = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) { before += w < wave ? s_wcnt[w] : 0; chunk += s_wcnt[w]; }
    base += chunk;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// Bitonic sort, ascending, of n_pow2 (uniform, a power of two) keys in LDS; the caller pads with ~0ull and passes a barrier
// after filling.  Every step ends in a barrier, so the sorted keys may be read at once.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort(unsigned long long *keys, int n_pow2) {
    for (int k = 2; k <= n_pow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n_pow2; i += THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = keys[i], y = keys[l];
                    const bool up = ((i & k) == 0);
                    if ((x > y) == up) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// The bin of a 256-bin histogram at which the running count, walking from bin 255 down (FROM_TOP) or from bin 0 up, first
// reaches `rank`: wave 0 only (threadIdx.x < 64), four bins per lane and a shuffle prefix over the lanes.  Exactly one lane
// finds it and leaves s_tmp = {bin, rank within the bin, count of the bin}.
template <bool FROM_TOP>
__device__ __forceinline__ void radix_pick_bin(int rank, const unsigned *s_hist /*[256]*/, int *s_tmp /*[3]*/) {
    const int l = threadIdx.x;
    int h[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = 4 * l + i;
        h[i] = (int)s_hist[FROM_TOP ? 255 - t : t];
        sum += h[i];
    }
    const int inc = wave_incl_scan(sum);
    int cum = inc - sum;
    if (cum < rank && rank <= inc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (cum + h[i] >= rank) {
                const int t = 4 * l + i;
                s_tmp[0] = FROM_TOP ? 255 - t : t;
                s_tmp[1] = rank - cum;
                s_tmp[2] = h[i];
                break;
            }
            cum += h[i];
        }
    }
}

// MSB-first radix select, 8 bits per pass, over BITS-bit unsigned keys: the key of rank `rank` (1-based, uniform, at most the
// number of candidates) counting from the largest key (FROM_TOP) or from the smallest.  *n_same = how many candidates carry
// exactly that key, *rank_in_same = how many of them are needed to reach `rank`: n_same > rank_in_same means a tie at the cut,
// which the callers break by a second select on the index, from the bottom (the lower index wins).
// The candidates are the caller's: once per pass the select calls visit(count), and the visitor calls count(key) for each
// candidate key of this thread, every candidate exactly once over the workgroup, the same ones in every pass.  Keys of 32 bits
// or fewer are handled as unsigned, wider ones as unsigned long long.
// Four barriers per pass: histogram cleared / counted / bin picked / s_tmp read (so the next pass, or the next select on the
// same LDS, may overwrite it).
template <int BITS, bool FROM_TOP, int THREADS, typename Visit>
__device__ __forceinline__ unsigned long long radix_select(int rank, Visit visit, unsigned *s_hist /*[256]*/, int *s_tmp /*[3]*/,
                                                           int *n_same, int *rank_in_same) {
    static_assert(BITS % 8 == 0 && BITS >= 8 && BITS <= 64, "whole 8-bit digits");
    using Key = std::conditional_t<(BITS > 32), unsigned long long, unsigned>;
    Key prefix = 0, mask = 0;
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += THREADS) s_hist[i] = 0;
        __syncthreads();
        visit([=](Key k) {
            if ((k & mask) == prefix) atomicAdd(&s_hist[(unsigned)(k >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (threadIdx.x < 64) radix_pick_bin<FROM_TOP>(rank, s_hist, s_tmp);
        __syncthreads();
        prefix |= (Key)(unsigned)s_tmp[0] << shift;
        mask |= (Key)255u << shift;
        rank = s_tmp[1];
        __syncthreads();
    }
    *n_same = s_tmp[2];
    *rank_in_same = rank;
    return prefix;
}

}  // namespace
}  // namespace balf
