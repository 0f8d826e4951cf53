// NMS score maps on gfx950: the two remaining NMS protocols of the reference's evaluation configs, batched.
//
//   GREEDY  apply_nms_fast / get_nms_score_map_from_score_map (benchmark_test/repeatability_tools.py:25-100): the greedy
//           (2d+1)^2 sweep in descending score order, the survivors >= conf_thresh written into a zero map.  A pixel
//           suppresses only pixels behind it in the order, so one below conf_thresh suppresses only pixels that are dropped
//           anyway: the map is the greedy NMS of the candidates >= conf_thresh, i.e. the kept list of nms_fast.hip, scattered.
//   BOX     box_nms (:227-255): every pixel >= min_prob is a size x size box around itself, torchvision's nms keeps a box iff
//           no kept box has IoU > iou with it.  All boxes are equal squares on the integer grid, so the IoU of two of them is a
//           function of their offset alone and the protocol is the greedy sweep with the FOOTPRINT F = {offset : IoU > iou}
//           in place of the square window.  The caller computes F once per call (float32, the reference's box_iou) and passes it
//           as a bit table in the kernels' argument block: no kernel evaluates an IoU.
//
// The BOX kernels are the exact parallel form of the sweep that nms_fast.hip's header describes, with the footprint as data:
//   repeat { keep: an alive candidate whose key is the largest of the alive candidates inside its footprint is KEPT;
//            kill: an alive candidate with a newly kept one inside its footprint dies (F is symmetric and holds the centre:
//                  the same table serves both tests and a kept candidate leaves the alive set) } until nobody is alive.
// Priority = nms_key.h: the higher score, then the lower raster index.  State in HBM: one alive bit and one kept-in-this-round
// bit per pixel ([B][H][ceil(W/64)] words), per image two ping-pong lists of the 64 x 32 tiles that still hold candidates, and
// per tile the round in which its kept words were last written (a tile that left the list keeps stale words: they are read
// only when that round is the current one).  A round is two launches over the lists; the keys (tile + a halo of `radius`)
// exist in LDS only.  TERMINATION: the largest alive key of an image is the largest inside its own footprint, so every round
// keeps at least one candidate of every image that has one and the alive set shrinks: at most H * W rounds.  BOX_ROUNDS rounds
// are enqueued as launches (one on an empty list returns at once); box_tail_kernel, ONE workgroup per image looping rounds
// over its own list, finishes what is left.  No workgroup waits for another one; no spin loop, no float atomic.
// Then (both protocols): the optional cut at the keep_top_k best survivors (a 64-bit radix select over the keys: they are
// distinct, so the cut is one key) and the scatter into the zero-filled map.
#include "block_ops.h"
#include "common.h"
#include "nms_key.h"

size_t balf_greedy_survivors_bytes(int B, int H, int W);                                   // nms_fast.hip
int balf_greedy_survivors_launch(const float *prob_dev, int B, int H, int W, float conf_thresh, int dist_thresh, void *workspace_dev,
                                 hipStream_t st, const int2 **surv, const int **counts);

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;
using balf::kmax;
using balf::make_key;
using balf::wave_incl_scan;
using balf::wave_sum;

constexpr int TW = 64, TH = 32;                      // tile: one 64-bit word wide
constexpr int R_MAX = BALF_NMS_MAP_MAX_RADIUS;       // 16 (<= TH, <= TW: a halo reaches the adjacent tiles only)
constexpr int RS = TW + 2 * R_MAX + 1;               // LDS row stride in keys: 97 = 194 dwords = 2 mod 64 -> a row of keys is conflict-free
constexpr int RH_MAX = TH + 2 * R_MAX;               // 64 region rows
constexpr int KTHREADS = 256;                        // keep kernels, tail kernel
constexpr int LTHREADS = 64;                         // kill kernel: one wave per tile
constexpr int BOX_ROUNDS = 8;                        // rounds enqueued as launches before the per-image tail
constexpr int SEL_THREADS = 1024;                    // the keep_top_k cut: one workgroup per image
constexpr int CTR_STRIDE = 64;                       // one 256-byte line per counter (see nms_fast.hip)

struct Footprint { u64 row[2 * R_MAX + 1]; };        // bit dc + radius of row dr + radius; by value in the argument block

struct BoxArgs {
    const float *src;             // [B, H, W]
    int H, W;
    float conf;
    int R;                        // footprint radius
    int B, ntx, nty;
    u64 *alive;                   // [B, H, ntx]
    u64 *kept;                    // [B, H, ntx] kept in the round kept_round says
    int *kept_round;              // [B, nty * ntx] the round whose keep pass wrote the tile's kept words (0: none yet)
    int *list;                    // [2, B, nty * ntx] live tiles: list[r & 1] is read by round r, written by round r - 1
    int *ctr;                     // counters, CTR_STRIDE ints apart: survivors [B], list lengths [2, B]
    int2 *surv;                   // [B, H * W] kept points (flat index, score bits), appended as they are kept; the counter says how many
};
// The arguments as ONE image sees them: every per-image base is formed once per kernel, and the tile functions below take no
// image index (the tail kernel, which inlines both passes, then holds one pointer per array and fits its scalar registers).
__device__ __forceinline__ BoxArgs image_view(BoxArgs a, int b) {
    const long tiles = (long)a.nty * a.ntx;
    a.src += (long)b * a.H * a.W;
    a.alive += (long)b * a.H * a.ntx;
    a.kept += (long)b * a.H * a.ntx;
    a.kept_round += b * tiles;
    a.list += b * tiles;                                      // list[parity] of the image: a.list + parity * B * tiles
    a.ctr += (long)b * CTR_STRIDE;
    a.surv += (long)b * a.H * a.W;
    return a;
}
__device__ __forceinline__ int *ctr_surv(const BoxArgs &a) { return a.ctr; }
__device__ __forceinline__ int *ctr_list(const BoxArgs &a, int parity) { return a.ctr + (long)(1 + parity) * a.B * CTR_STRIDE; }
__device__ __forceinline__ int *tile_list(const BoxArgs &a, int parity) { return a.list + (long)parity * a.B * a.nty * a.ntx; }

struct KeepLds {
    double key[RH_MAX * RS];       // keys of the tile and its halo; +0: no alive candidate there
    u64 words[RH_MAX * 3];         // alive words of the region rows: left neighbour / own / right neighbour tile column
    u64 kw[TH], aw[TH];            // kept / alive words of the tile's rows
};
struct KillLds {
    u64 lo[RH_MAX], hi[RH_MAX];    // per region row 128 kept bits: bit k = column tx0 - 16 + k
};

// Keep pass of one tile: writes the tile's words of the `kept` map (and, in round 1, of the `alive` map: the candidates come
// straight from the score map).  `a` is the image's view.  All threads of the workgroup take part (blockDim.x = KTHREADS).
template <bool FIRST>
__device__ __forceinline__ void keep_tile(const BoxArgs &a, const Footprint &fp, KeepLds &s, int tile, int round) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx, ty0 = tyi * TH, tx0 = txi * TW;
    const int R = a.R, RH = TH + 2 * R, RW = TW + 2 * R, ry0 = ty0 - R, rx0 = tx0 - R;
    const float *img = a.src;
    __syncthreads();                                  // the workgroup's previous tile is done with the LDS
    if (!FIRST) {
        for (int i = tid; i < RH * 3; i += KTHREADS) {
            const int r = i / 3, j = i - r * 3, y = ry0 + r, wx = txi - 1 + j;
            s.words[i] = (y >= 0 && y < a.H && wx >= 0 && wx < a.ntx) ? a.alive[(long)y * a.ntx + wx] : 0ull;
        }
        __syncthreads();
    }
    // one flat loop over the region: every thread has RH * RW / 256 independent loads in flight (a wave per row with the lanes
    // along x needs no index division but keeps two loads per lane in flight: measured 0.94 ms against 0.84 ms for round 1)
    for (int i = tid; i < RH * RW; i += KTHREADS) {
        const int r = i / RW, c = i - r * RW, y = ry0 + r, x = rx0 + c;
        double k = 0.0;
        if (FIRST) {
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                const float v = img[(long)y * a.W + x];
                if (v >= a.conf) k = make_key(v, y * a.W + x);
            }
        } else {
            const int bit = c + 64 - R;               // bit 0 of word 0 = column tx0 - 64; an alive bit is inside the image
            if ((s.words[r * 3 + (bit >> 6)] >> (bit & 63)) & 1ull) k = make_key(img[(long)y * a.W + x], y * a.W + x);
        }
        s.key[r * RS + c] = k;
    }
    __syncthreads();
    // wave wv: tile rows 8 wv .. 8 wv + 7, lanes along x.  The footprint loops are uniform: the row words come from the
    // argument block through scalar loads, the keys of a row offset are 64 consecutive doubles.
#pragma unroll 1
    for (int j = 0; j < TH / (KTHREADS / 64); ++j) {
        const int r = wv * (TH / (KTHREADS / 64)) + j;
        const double own = s.key[(r + R) * RS + lane + R];
        const u64 am = __ballot(own != 0.0);
        u64 km = 0ull;
        if (am) {                                     // uniform
            double m = 0.0;
            for (int q = 0; q <= 2 * R; ++q) {
                u64 fw = fp.row[q];
                const double *rowp = s.key + (r + q) * RS + lane;      // column lane - R + bit of the region = tile column lane + dc
                while (fw) {
                    const int bit = __builtin_ctzll(fw);
                    fw &= fw - 1ull;
                    m = kmax(m, rowp[bit]);
                }
            }
            km = __ballot(own != 0.0 && m == own);    // the centre is in the footprint: m >= own
        }
        if (lane == 0) { s.kw[r] = km; s.aw[r] = am; }
    }
    __syncthreads();
    if (tid < TH && ty0 + tid < a.H) {
        const long wi = (long)(ty0 + tid) * a.ntx + txi;
        a.kept[wi] = s.kw[tid];
        if (FIRST) a.alive[wi] = s.aw[tid];
    }
    if (tid == 0) a.kept_round[tile] = round;
}

// Kill pass of one tile whose keep pass ran in this round.  Wave 0 of the workgroup does the work; every thread must call it
// (two barriers).
__device__ __forceinline__ void kill_tile(const BoxArgs &a, const Footprint &fp, KillLds &s, int tile, int round) {
    const int tid = threadIdx.x;
    const int tyi = tile / a.ntx, txi = tile - tyi * a.ntx, ty0 = tyi * TH, tx0 = txi * TW;
    const int R = a.R, RH = TH + 2 * R;
    const float *img = a.src;
    __syncthreads();                                  // the previous tile of this workgroup is done with the LDS
    if (tid < RH) {
        const int y = ty0 - R + tid;
        u64 L = 0ull, M = 0ull, Rw = 0ull;
        if (y >= 0 && y < a.H) {
            const int *kr = a.kept_round + (y / TH) * a.ntx;
            const u64 *row = a.kept + (long)y * a.ntx;
            if (txi > 0 && kr[txi - 1] == round) L = row[txi - 1];
            if (kr[txi] == round) M = row[txi];
            if (txi + 1 < a.ntx && kr[txi + 1] == round) Rw = row[txi + 1];
        }
        s.lo[tid] = (L >> 48) | (M << 16);
        s.hi[tid] = (M >> 48) | (Rw << 16);
    }
    u64 al = 0ull, kp = 0ull;
    if (tid < TH && ty0 + tid < a.H) {
        const long wi = (long)(ty0 + tid) * a.ntx + txi;
        al = a.alive[wi];
        kp = a.kept[wi];
    }
    __syncthreads();
    if (tid >= 64) return;
    u64 v = 0ull;                                      // bit c: a newly kept point inside the footprint of tile column c
    if (tid < TH) {
        for (int q = 0; q <= 2 * R; ++q) {
            u64 fw = fp.row[q];
            const u128 t = ((u128)s.hi[tid + q] << 64) | (u128)s.lo[tid + q];
            while (fw) {
                const int bit = __builtin_ctzll(fw);
                fw &= fw - 1ull;
                v |= (u64)(t >> (16 - R + bit));       // column tx0 + c + dc, dc = bit - R
            }
        }
    }
    // newly kept points onto the survivor list: one atomic per tile
    const int nk = __popcll(kp);
    const int incl = wave_incl_scan(nk);
    const int total = __shfl(incl, 63);
    if (total) {
        int base = 0;
        if (tid == 0) base = atomicAdd(ctr_surv(a), total);
        base = __shfl(base, 0);
        int2 *out = a.surv + base + incl - nk;
        const int y = ty0 + tid;
        while (kp) {
            const int x = tx0 + __builtin_ctzll(kp);
            kp &= kp - 1ull;
            *out++ = make_int2(y * a.W + x, (int)__float_as_uint(img[(long)y * a.W + x]));
        }
    }
    const u64 na = al & ~v;                            // the kept ones themselves and whoever they suppress
    if (na != al) a.alive[(long)(ty0 + tid) * a.ntx + txi] = na;
    const int alive = wave_sum(__popcll(na));
    if (tid == 0 && alive != 0) {
        const int nxt = (round + 1) & 1;
        tile_list(a, nxt)[atomicAdd(ctr_list(a, nxt), 1)] = tile;
    }
}

// round 1: every tile, one workgroup each
__global__ __launch_bounds__(KTHREADS) void box_keep_first_kernel(BoxArgs all, Footprint fp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    keep_tile<true>(image_view(all, blockIdx.y), fp, *reinterpret_cast<KeepLds *>(smem), blockIdx.x, 1);
}

__global__ __launch_bounds__(KTHREADS) void box_keep_kernel(BoxArgs all, Footprint fp, int round) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    KeepLds &s = *reinterpret_cast<KeepLds *>(smem);
    const BoxArgs a = image_view(all, blockIdx.y);
    const int cur = round & 1;
    const int n = *ctr_list(a, cur);
    if (blockIdx.x == 0 && threadIdx.x == 0) *ctr_list(a, cur ^ 1) = 0;          // this round's kill pass fills it
    const int *list = tile_list(a, cur);
    for (int i = blockIdx.x; i < n; i += gridDim.x) keep_tile<false>(a, fp, s, list[i], round);
}

template <bool FIRST>
__global__ __launch_bounds__(LTHREADS) void box_kill_kernel(BoxArgs all, Footprint fp, int round) {
    __shared__ KillLds s;
    const BoxArgs a = image_view(all, blockIdx.y);
    if (FIRST) {
        kill_tile(a, fp, s, blockIdx.x, 1);
        return;
    }
    const int cur = round & 1;
    const int n = *ctr_list(a, cur);
    const int *list = tile_list(a, cur);
    for (int i = blockIdx.x; i < n; i += gridDim.x) kill_tile(a, fp, s, list[i], round);
}

// Whatever the enqueued rounds left alive: one workgroup per image runs further rounds over the image's own tile list.  The
// workgroup reads what it wrote itself in the previous pass (bit maps, lists, kept_round): device-scope fences around the
// barriers, the counters through atomic loads.
__global__ __launch_bounds__(KTHREADS) void box_tail_kernel(BoxArgs all, Footprint fp, int round0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    KeepLds &sk = *reinterpret_cast<KeepLds *>(smem);
    KillLds &sl = *reinterpret_cast<KillLds *>(smem + sizeof(KeepLds));
    const BoxArgs a = image_view(all, blockIdx.x);
    const int tid = threadIdx.x;
    for (int round = round0;; ++round) {
        const int cur = round & 1;
        const int n = __hip_atomic_load(ctr_list(a, cur), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) break;                                    // uniform: every thread reads the same settled word
        __syncthreads();
        if (tid == 0) __hip_atomic_store(ctr_list(a, cur ^ 1), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int *list = tile_list(a, cur);
        // (the list was written by this workgroup in the previous pass: read through agent-scope loads, like the counters)
        for (int i = 0; i < n; ++i)
            keep_tile<false>(a, fp, sk, __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), round);
        __threadfence();
        __syncthreads();
        __threadfence();
        for (int i = 0; i < n; ++i)
            kill_tile(a, fp, sl, __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), round);
        __threadfence();
        __syncthreads();
        __threadfence();
    }
}

// ---- both protocols: the cut at the keep_top_k best survivors and the scatter ------------------------------------------------------
__device__ __forceinline__ u64 entry_key(int2 e) { return ((u64)(unsigned)e.y << 32) | (u64)(0xffffffffu - (unsigned)e.x); }

// counts[b * count_stride] survivors of image b (contiguous from the greedy rounds, one per counter line from the box rounds).
// cut[b] = the key of image b's K-th best survivor (score descending, raster index ascending), 0 where it has at most K
__global__ __launch_bounds__(SEL_THREADS) void map_cut_kernel(const int2 *surv_all, const int *counts, int count_stride, long cap, int K,
                                                             u64 *cut) {
    __shared__ unsigned s_hist[256];
    __shared__ int s_tmp[4];
    const int b = blockIdx.x;
    const int2 *surv = surv_all + (long)b * cap;
    const int n = balf::clamp_count(counts, (long)b * count_stride, (int)cap);
    if (n <= K) {                                             // uniform
        if (threadIdx.x == 0) cut[b] = 0ull;
        return;
    }
    int n_same, need_same;                                    // the keys are distinct: 1 and 1
    const u64 c = balf::radix_select<64, true, SEL_THREADS>(
        K, [&](auto count) { for (int i = threadIdx.x; i < n; i += SEL_THREADS) count(entry_key(surv[i])); }, s_hist, s_tmp, &n_same,
        &need_same);
    if (threadIdx.x == 0) cut[b] = c;
}

// out is zero-filled before: the survivors at or above the cut get their score; count_out[b] = how many those are
__global__ __launch_bounds__(256) void map_scatter_kernel(const int2 *surv_all, const int *counts, int count_stride, long cap, int K,
                                                          const u64 *cut, float *out, int32_t *count_out) {
    const int b = blockIdx.y;
    const int2 *surv = surv_all + (long)b * cap;
    const int n = balf::clamp_count(counts, (long)b * count_stride, (int)cap);
    const u64 c = cut ? cut[b] : 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int2 e = surv[i];
        if (entry_key(e) >= c && (unsigned)e.x < (unsigned long)cap) out[(long)b * cap + e.x] = __int_as_float(e.y);
    }
    if (count_out && blockIdx.x == 0 && threadIdx.x == 0) count_out[b] = (cut && n > K) ? K : n;
}

struct Layout {
    u64 *cut;                     // [B]
    void *greedy;                 // GREEDY: the workspace of balf_greedy_survivors_launch
    int *ctr, *keptr, *list;                // BOX
    u64 *alive, *kept;
    int2 *surv;
    size_t zero_bytes;            // ctr, keptr: cleared per call
    size_t total;
};
Layout layout(int B, int H, int W, int protocol, void *base = nullptr) {
    Layout l{};
    WorkspaceCursor c{static_cast<char *>(base), 0};
    l.cut = c.take<u64>((size_t)B * sizeof(u64));
    if (protocol == BALF_NMS_MAP_GREEDY) {
        l.greedy = c.take_exact<char>(balf_greedy_survivors_bytes(B, H, W));
    } else {
        const size_t ntx = balf_ceil_div(W, TW), nty = balf_ceil_div(H, TH), tiles = ntx * nty;
        const size_t per_tile = (size_t)B * tiles * sizeof(int), map = (size_t)B * H * ntx * sizeof(u64);
        const size_t at = c.used;
        // INVARIANT the fill of balf_nms_score_map rests on: ctr and keptr follow each other
        l.ctr = c.take<int>((size_t)3 * B * CTR_STRIDE * sizeof(int));
        l.keptr = c.take<int>(per_tile);
        l.zero_bytes = c.used - at;
        l.list = c.take<int>(2 * per_tile);
        l.alive = c.take<u64>(map);
        l.kept = c.take<u64>(map);
        l.surv = c.take_exact<int2>((size_t)B * H * W * sizeof(int2));
    }
    l.total = c.used;
    return l;
}

int check_sizes(int B, int H, int W, int protocol) {
    if (protocol != BALF_NMS_MAP_GREEDY && protocol != BALF_NMS_MAP_BOX) return BALF_ERR_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return BALF_ERR_ARG;      // blockIdx.y
    if ((long)H * W > 0x7fffffffL) return BALF_ERR_SHAPE;
    if ((long)balf_ceil_div(W, TW) * balf_ceil_div(H, TH) * B > 0x7fffffffL) return BALF_ERR_SHAPE;
    return BALF_OK;
}

// the centre suppresses, nothing lies outside the (2 radius + 1)^2 square, and F is symmetric (one table for both tests)
bool footprint_ok(const uint64_t *rows, int radius) {
    const int n = 2 * radius + 1;
    for (int r = 0; r < n; ++r) {
        if (rows[r] >> n) return false;
        for (int c = 0; c < n; ++c)
            if (((rows[r] >> c) & 1u) != ((rows[n - 1 - r] >> (n - 1 - c)) & 1u)) return false;
    }
    return (rows[radius] >> radius) & 1u;
}

int box_survivors(const float *prob_dev, int B, int H, int W, float conf, const uint64_t *rows, int radius, const Layout &l,
                  hipStream_t st) {
    const int ntx = balf_ceil_div(W, TW), nty = balf_ceil_div(H, TH), tiles = ntx * nty;
    BoxArgs a{prob_dev, H, W, conf, radius, B, ntx, nty, l.alive, l.kept, l.keptr, l.list, l.ctr, l.surv};
    Footprint fp{};
    for (int r = 0; r <= 2 * radius; ++r) fp.row[r] = rows[r];
    if (balf_fill_u32(l.ctr, 0u, l.zero_bytes / 4, st) != BALF_OK) return BALF_ERR_LAUNCH;
    constexpr int keep_lds = (int)sizeof(KeepLds), tail_lds = (int)(sizeof(KeepLds) + sizeof(KillLds));
    static_assert(sizeof(KeepLds) % 16 == 0 && 3 * sizeof(KeepLds) <= 160 * 1024, "three keep workgroups per CU");
    if (!balf_allow_dynamic_lds<box_keep_first_kernel>(keep_lds) || !balf_allow_dynamic_lds<box_keep_kernel>(keep_lds) ||
        !balf_allow_dynamic_lds<box_tail_kernel>(tail_lds))
        return BALF_ERR_LAUNCH;
    hipLaunchKernelGGL(box_keep_first_kernel, dim3(tiles, B), dim3(KTHREADS), keep_lds, st, a, fp);
    hipLaunchKernelGGL(box_kill_kernel<true>, dim3(tiles, B), dim3(LTHREADS), 0, st, a, fp, 1);
    BALF_LAUNCH_CHECK();
    // rounds 2.. over the lists: the workgroups stride over a list, so a grid smaller than it still covers it
    const int gk = tiles < 1024 / B + 16 ? tiles : 1024 / B + 16;
    const int gl = tiles < 16384 / B + 64 ? tiles : 16384 / B + 64;
    for (int r = 2; r <= BOX_ROUNDS; ++r) {
        hipLaunchKernelGGL(box_keep_kernel, dim3(gk, B), dim3(KTHREADS), keep_lds, st, a, fp, r);
        hipLaunchKernelGGL(box_kill_kernel<false>, dim3(gl, B), dim3(LTHREADS), 0, st, a, fp, r);
    }
    BALF_LAUNCH_CHECK();
    hipLaunchKernelGGL(box_tail_kernel, dim3(B), dim3(KTHREADS), tail_lds, st, a, fp, BOX_ROUNDS + 1);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}

}  // namespace

extern "C" int balf_nms_score_map_sizes(int B, int H, int W, int protocol, size_t *workspace_bytes) {
    if (!workspace_bytes) return BALF_ERR_ARG;
    const int rc = check_sizes(B, H, W, protocol);
    if (rc != BALF_OK) return rc;
    *workspace_bytes = layout(B, H, W, protocol).total;
    return BALF_OK;
}

extern "C" int balf_nms_score_map(const float *prob_dev, int B, int H, int W, int protocol, float conf_thresh, int dist_thresh,
                                  const uint64_t *footprint, int radius, int keep_top_k, float *out_dev, int32_t *count_dev,
                                  void *workspace_dev, size_t workspace_bytes, void *stream) {
    int rc = check_sizes(B, H, W, protocol);
    if (rc != BALF_OK) return rc;
    if (!(conf_thresh > 0.0f)) return BALF_ERR_ARG;
    if (protocol == BALF_NMS_MAP_GREEDY) {
        if (dist_thresh < 1 || dist_thresh > R_MAX) return BALF_ERR_ARG;
    } else {
        if (radius < 0 || radius > R_MAX || !footprint || !footprint_ok(footprint, radius)) return BALF_ERR_ARG;
    }
    if (!prob_dev || !out_dev || !workspace_dev) return BALF_ERR_ARG;
    const Layout l = layout(B, H, W, protocol, workspace_dev);
    if (workspace_bytes < l.total) return BALF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long cap = (long)H * W;

    const int2 *surv = l.surv;
    const int *counts = l.ctr;                                // the survivor counters of the box rounds
    const int stride = protocol == BALF_NMS_MAP_GREEDY ? 1 : CTR_STRIDE;
    if (protocol == BALF_NMS_MAP_GREEDY)
        rc = balf_greedy_survivors_launch(prob_dev, B, H, W, conf_thresh, dist_thresh, l.greedy, st, &surv, &counts);
    else
        rc = box_survivors(prob_dev, B, H, W, conf_thresh, footprint, radius, l, st);
    if (rc != BALF_OK) return rc;

    if (balf_fill_u32(out_dev, 0u, (size_t)B * cap, st) != BALF_OK) return BALF_ERR_LAUNCH;
    const bool cut = keep_top_k > 0 && keep_top_k < cap;      // (at most H * W survive)
    if (cut) hipLaunchKernelGGL(map_cut_kernel, dim3(B), dim3(SEL_THREADS), 0, st, surv, counts, stride, cap, keep_top_k,
                                l.cut);
    const int gs = (int)(cap / 1024 < 1 ? 1 : (cap / 1024 > 128 ? 128 : cap / 1024));
    hipLaunchKernelGGL(map_scatter_kernel, dim3(gs, B), dim3(256), 0, st, surv, counts, stride, cap, keep_top_k,
                       cut ? l.cut : nullptr, out_dev, count_dev);
    BALF_LAUNCH_CHECK();
    return BALF_OK;
}
