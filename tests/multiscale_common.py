"""References and cases of the multi-scale edge tests (tests/test_multiscale_edges_host.py, tests/test_multiscale_edges_gpu.py).

Nothing here needs a GPU to import.  The pyramid reference is the two library functions balf_pyramid_level claims to
reproduce (scipy.ndimage.gaussian_filter, torch.nn.functional.interpolate), in float64, for ONE level from the exact fp32 array
the kernel read; `fp32_emulation_level` is the kernel's own arithmetic in NumPy float32 and shows that the bound the GPU test
asserts is reachable by correct fp32 code; `tile_choice` restates the host's choice of tile height and LDS size, so that the
case list can be checked to reach every branch of it."""
import math

import numpy as np
import torch

ULP = 2.0 ** -24                # the unit of every pyramid bound: the spacing of fp32 in [0.5, 1)
PYR_TX, PYR_LDS_MAX, PYR_MAX_RADIUS = 64, 64 * 1024, 8
MAX_TOPK = 16384


def blur_radius(sigma):
    """scipy's truncate = 4.0 (nan / <= 0: no blur, as the library's `sigma > 0.0 ? ... : 0`)."""
    return int(4.0 * sigma + 0.5) if sigma > 0.0 else 0


def pyramid_bound(sigma):
    """|kernel - float64| <= (4R + 12) 2^-24 for sources in [0, 1].  With u = 2^-24, the spacing of fp32 in [0.5, 1): a value
    in [0, 1] rounds by at most u / 2.  The taps are non-negative and sum to 1, so every partial sum of a pass stays in [0, 1]:
    the 2R+1 fused multiply-adds of a pass round by at most (2R+1) u / 2 together, the rounding of the taps to fp32 moves the
    sum by at most u / 2, and the first pass's error goes through the second with weight 1: (2R + 2) u for both passes, counted
    generously as (4R + 2) u (products rounded on their own, not fused).  The bilinear form on values in [0, 1]: 1 - l twice,
    four products, two inner sums, two outer products, one sum, each <= u / 2, plus the rounding of the two lambdas (u / 2
    times a difference <= 1 each): under 7 u, counted as 10 u.  Total (4R + 12) u."""
    return (4 * blur_radius(sigma) + 12) * ULP


# ---- the pyramid level: float64 reference, fp32 emulation, tile choice ----------------------------------------------------------
def ref_pyramid_level(src_f32, sigma, h_out, w_out):
    """src_f32 [H,W,C] (or [H,W]) float32, the array the kernel read -> [h_out,w_out,C] float64: gaussian_filter(reflect,
    truncate 4) then F.interpolate(bilinear, align_corners=False), both in float64."""
    from scipy import ndimage
    src = np.asarray(src_f32)
    assert src.dtype == np.float32
    x = src.astype(np.float64)
    if x.ndim == 2:
        x = x[..., None]
    if blur_radius(sigma) > 0:         # radius 0 (sigma = 0.1): scipy's kernel is the single tap 1.0, the identity
        x = np.stack([ndimage.gaussian_filter(x[..., c], sigma=float(sigma), mode="reflect", truncate=4.0)
                      for c in range(x.shape[2])], axis=-1)
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]
    y = torch.nn.functional.interpolate(t, size=(int(h_out), int(w_out)), mode="bilinear", align_corners=False)
    return y[0].numpy().transpose(1, 2, 0)


def _axis(n_in, n_out):
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0).astype(np.float32)          # lambda: float64 coordinate, rounded to fp32 once


def fp32_emulation_level(src_f32, sigma, h_out, w_out):
    """The kernel's arithmetic in NumPy float32, in its order: taps exp(-k^2 / 2 sigma^2) / sum in float64 rounded to fp32,
    row pass then column pass with acc = fma(tap, v, acc) from k = -R upwards (the product of two fp32 is exact in float64, so
    float64 add + one rounding is the fused operation up to a double rounding), half-sample symmetric border on both axes
    before the row pass, then (1-ly)((1-lx) v00 + lx v01) + ly((1-lx) v10 + lx v11) in fp32."""
    x = np.asarray(src_f32)
    assert x.dtype == np.float32
    if x.ndim == 2:
        x = x[..., None]
    h, w = x.shape[:2]
    r = blur_radius(sigma)
    if r > 0:
        k = np.arange(-r, r + 1, dtype=np.float64)
        t = np.exp(-0.5 * k * k / (float(sigma) * float(sigma)))
        taps = (t / t.sum()).astype(np.float32)
        p = np.pad(x, ((r, r), (r, r), (0, 0)), mode="symmetric")
        acc = np.zeros((h + 2 * r, w, x.shape[2]), np.float32)
        for j in range(2 * r + 1):
            acc = (acc.astype(np.float64) + np.float64(taps[j]) * p[:, j:j + w].astype(np.float64)).astype(np.float32)
        p, acc = acc, np.zeros_like(x)
        for j in range(2 * r + 1):
            acc = (acc.astype(np.float64) + np.float64(taps[j]) * p[j:j + h].astype(np.float64)).astype(np.float32)
        x = acc
    y0, y1, ly = _axis(h, h_out)
    x0, x1, lx = _axis(w, w_out)
    ly, lx = ly[:, None, None], lx[None, :, None]
    one = np.float32(1.0)
    top = (one - lx) * x[y0][:, x0] + lx * x[y0][:, x1]
    bot = (one - lx) * x[y1][:, x0] + lx * x[y1][:, x1]
    out = (one - ly) * top + ly * bot
    assert out.dtype == np.float32
    return out


def tile_choice(h_in, w_in, sigma, h_out, w_out):
    """The host's tile choice restated -> (ty, lds_bytes), or (0, None) when the call is refused: the footprint width of a
    64-pixel output row, then the tile height from 8 down until two float planes fit in 64 KB."""
    r = blur_radius(sigma)
    sc_y, sc_x = float(h_in) / float(h_out), float(w_in) / float(w_out)
    fw = int(math.ceil((PYR_TX - 1) * sc_x)) + 3 + 2 * r
    for ty in (8, 4, 2, 1):
        fh = int(math.ceil((ty - 1) * sc_y)) + 3 + 2 * r
        if 2 * fh * fw * 4 <= PYR_LDS_MAX:
            return ty, 2 * fh * fw * 4
    return 0, None


# ---- the pyramid cases ---------------------------------------------------------------------------------------------------------
# kind: 'u8gray' uint8 [B,H,W]; 'u8rgb' uint8 [B,H,W,3]; 'f32rgb' fp32 [B,H,W,3]; 'level1' / 'level3': a padded level (gray /
# colour) that an identity call of the kernel wrote from the uint8 image and the test read back
def _c(name, kind, h_in, w_in, sigma, h_out, w_out, seed=None):
    return dict(name=name, kind=kind, h_in=h_in, w_in=w_in, sigma=sigma, h_out=h_out, w_out=w_out,
                seed=len(name) * 131 + h_in * 7 + w_in if seed is None else seed)


SIGMA_DEFAULT = 2.0 * math.sqrt(2.0) / 6.0      # 0.4714: R = 2, the workload's own setting

PYRAMID_GROUPS = {
    # shrunk tiles and the launch with more than 48 KB of LDS; the two 'fits' cases are the largest reductions that are accepted
    "tiles": [
        _c("ty1_r8_60k", "u8gray", 200, 400, 2.0, 34, 67),
        _c("ty4_r2", "u8rgb", 160, 256, 0.5, 40, 64),
        _c("ty2_r4", "f32rgb", 151, 323, 1.0, 30, 64),
        _c("ty8_r0_over48k", "level3", 96, 512, 0.0, 24, 128),
        _c("fits_r8", "level1", 16, 653, 2.0, 8, 100),
        _c("fits_r0", "u8rgb", 4, 432, 0.0, 2, 10),
    ],
    # reflect with several wraps: the blur radius exceeds the image
    "reflect": [_c(f"h{h}_r{r}", kind, h, 37, sg, h + 1, 29)
                for (h, kind) in ((1, "u8gray"), (2, "u8rgb"), (3, "f32rgb"), (5, "level1"))
                for (r, sg) in ((8, 2.0), (2, 0.5))]
    + [_c("w1_r8", "level3", 9, 1, 2.0, 5, 3), _c("w1_r2", "f32rgb", 9, 1, 0.5, 5, 3)],
    "upsampling": [
        _c("up_64_to_181", "u8gray", 64, 64, 0.0, 181, 181),
        _c("up_7x9_to_64x100", "f32rgb", 7, 9, SIGMA_DEFAULT, 64, 100),
        _c("up_1x1_to_5x5", "u8rgb", 1, 1, 0.0, 5, 5),
    ],
    "anisotropic": [_c("aniso_120x50_to_31x97", "u8rgb", 120, 50, 1.0, 31, 97)],
    # `left` / `top` through all phases, padding-only tiles, partly padded tiles, one-column remainders; one source for all
    "sweep": [_c(f"sweep_{ho}x{wo}", "u8gray" if (wo + ho) % 2 else "u8rgb", 90, 140, SIGMA_DEFAULT, ho, wo, seed=90140)
              for wo in list(range(61, 69)) + list(range(125, 132)) for ho in range(7, 11)],
    "src_level": [
        _c("level_odd_gray", "level1", 333, 517, SIGMA_DEFAULT, 236, 366),
        _c("level_odd_rgb", "level3", 333, 517, SIGMA_DEFAULT, 236, 366),
    ],
    "sigma": [
        _c("sigma_0p1_identity", "f32rgb", 40, 56, 0.1, 29, 40),
        _c("sigma_2p1_r8", "u8gray", 40, 56, 2.1, 29, 40),
    ],
}
PYRAMID_CASES = [c for g in PYRAMID_GROUPS.values() for c in g]

# refused: the reduction one source column past 'fits_r8' / 'fits_r0', and the sigma edges
REFUSED_CASES = [
    _c("past_r8", "u8gray", 16, 654, 2.0, 8, 100),
    _c("past_r0", "u8rgb", 4, 433, 0.0, 2, 10),
    _c("sigma_2p2_r9", "u8gray", 40, 56, 2.2, 29, 40),
    _c("sigma_64", "u8gray", 40, 56, 64.0, 29, 40),
    _c("sigma_nan", "u8gray", 40, 56, float("nan"), 29, 40),
]

PYR_BATCH = 2


def case_channels(case):
    return 1 if case["kind"] in ("u8gray", "level1") else 3


def case_source(case, b=PYR_BATCH):
    """-> (host array for the device, base [B,H,W,C] float32): `base` is the exact fp32 array the kernel reads -- value / 255
    in float64 rounded to fp32 for uint8, and what an identity level holds (bit for bit: test_multiscale_gpu.py) for a level."""
    rng = np.random.default_rng(case["seed"])
    h, w, ch = case["h_in"], case["w_in"], case_channels(case)
    if case["kind"] == "f32rgb":
        src = rng.random((b, h, w, 3), dtype=np.float32)
        return src, src
    shape = (b, h, w) if ch == 1 else (b, h, w, 3)
    src = np.clip(rng.normal(128, 60, shape), 0, 255).astype(np.uint8)
    base = (src.astype(np.float64) / 255.0).astype(np.float32).reshape(b, h, w, ch)
    return src, base


# ---- budgeted top-K ---------------------------------------------------------------------------------------------------------------
def ref_budget_k(cum_budget, taken, h, w, k_max):
    """The K balf_nms_topk_budget decides for an image."""
    return min(max(int(cum_budget) - int(taken), 0), int(k_max), int(h) * int(w))


# ---- merge --------------------------------------------------------------------------------------------------------------------------
def np_homography_points(points, h):
    """apply_homography_to_points in plain float64 NumPy: rows (x, y, radius, score) -> the warped point and the radius
    rescaled by the warp's local affine approximation."""
    p = np.asarray(points, np.float64).reshape(-1, 4)
    h = np.asarray(h, np.float64).reshape(9)
    x, y, r = p[:, 0], p[:, 1], p[:, 2]
    den = h[6] * x + h[7] * y + h[8]
    nx, ny = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5]
    fxdx, fxdy = h[0] / den - nx * h[6] / (den * den), h[1] / den - nx * h[7] / (den * den)
    fydx, fydy = h[3] / den - ny * h[6] / (den * den), h[4] / den - ny * h[7] / (den * den)
    tmp = r * r + np.float64(np.finfo(np.float32).eps)
    return np.stack([nx / den, ny / den, np.sqrt(tmp * np.abs(fxdx * fydy - fxdy * fydx)), p[:, 3]], axis=1)


def ref_merge(idx, score, count, widths, homographies, n, order_yx, k_max, mapper=np_homography_points):
    """One image's level lists idx / score [L,K], count [L] -> (rows [m,4] float64, m): counts clamped to [0, k_max], entries
    ordered by (score descending on the float value, level ascending, index ascending), the first n mapped through their
    level's homography by `mapper` (rows (x, y, 1, score) and a 3x3 matrix -> rows).  (zero rows, -1) when the clamped total
    exceeds min(L k_max, 16384)."""
    idx, score = np.asarray(idx), np.asarray(score)
    nl = idx.shape[0]
    cnt = np.clip(np.asarray(count, np.int64), 0, k_max)
    if int(cnt.sum()) > min(nl * k_max, MAX_TOPK):
        return np.zeros((0, 4)), -1
    lv = np.concatenate([np.full(int(c), l, np.int64) for l, c in enumerate(cnt)]) if nl else np.zeros(0, np.int64)
    ii = np.concatenate([idx[l, :int(c)].astype(np.int64) for l, c in enumerate(cnt)])
    ss = np.concatenate([score[l, :int(c)].astype(np.float32) for l, c in enumerate(cnt)])
    o = np.lexsort((ii, lv, -ss.astype(np.float64)))[:n]
    lv, ii, ss = lv[o], ii[o], ss[o]
    out = np.zeros((len(o), 4))
    for l in range(nl):
        m = lv == l
        if m.any():
            w = int(widths[l])
            pts = np.stack([(ii[m] % w).astype(np.float64), (ii[m] // w).astype(np.float64), np.ones(int(m.sum())),
                            ss[m].astype(np.float64)], axis=1)
            out[m] = np.asarray(mapper(pts, homographies[l])).reshape(-1, 4)
    if order_yx and len(out):
        out[:, [0, 1]] = out[:, [1, 0]]
    return out, len(o)


# ---- guard bands --------------------------------------------------------------------------------------------------------------------
GUARD, PAT = 4096, 0xA5


class Guarded:
    """`nbytes` usable bytes on the GPU between two 4 KB bands of a byte pattern; .ptr is what the library gets.  The usable
    bytes start as the same pattern (garbage for every type) unless `fill` is given."""

    def __init__(self, nbytes, fill=None, device="cuda:0"):
        self.n = int(nbytes)
        self.full = torch.full((2 * GUARD + self.n,), PAT, dtype=torch.uint8, device=device)
        if fill is not None:
            self.full[GUARD:GUARD + self.n] = fill
        self.ptr = self.full.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def view(self, dtype, shape):
        return self.full[GUARD:GUARD + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.full[:GUARD] == PAT).all()) and bool((self.full[GUARD + self.n:] == PAT).all())
