"""Shared by the pair-synthesis tests (test_pair_synth_host.py, test_pair_synth_gpu.py) and the recording script
(tests/golden/make_pair_synth_golden.py): access to tests/golden/pair_synth.npz, an integer NumPy restatement of
balf_synth_pairs' definition of the 8-bit warp (include/balf_hip.h) -- the FULL image, then the crop, the way the reference
does it --, the label path restated with the port's tie rule (higher prob first, then the lower row index), and the case
table."""
import functools
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_synth.npz")
IMAGE_SHAPES = ((96, 128), (80, 112))       # (h, w) of the two source photographs
PATCHES = (32, 64)
BATCHES = (1, 3, 17)
TOP_KS = (25, 0)                            # every case is recorded with both: the cut, and "keep all"


def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def images():
    """The two RGB source images (channels differ), regenerated from seeds."""
    from balf_amd.utils import synth
    out = []
    for i, (h, w) in enumerate(IMAGE_SHAPES):
        g = synth.synthetic_gray_u8(h, w, 700 + i)
        out.append(np.ascontiguousarray(np.stack([g, 255 - g, (g.astype(np.int64) * 2 // 3).astype(np.uint8)], axis=2)))
    return out


# ---- the case table -------------------------------------------------------------------------------------------------------
def _rot(h, w, deg, scale):
    c, s = np.cos(np.deg2rad(deg)) * scale, np.sin(np.deg2rad(deg)) * scale
    cx, cy = w / 2.0, h / 2.0
    return np.array([[c, s, (1 - c) * cx - s * cy], [-s, c, s * cx + (1 - c) * cy], [0.0, 0.0, 1.0]])


def _shift(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


MILD = np.array([[1.03, 0.04, -3.25], [-0.03, 0.98, 2.6], [6e-5, -4e-5, 1.0]])


def cases(patch):
    """name -> dict(image, inv_h (what cv2.warpPerspective is handed), win_src, win_dst (top, left), labels (kind, n),
    exact (the label warp is exact in any evaluation order)).  The destination image is src sampled at inv(inv_h) (x, y, 1)."""
    (ha, wa), (hb, wb) = IMAGE_SHAPES
    mid_a, mid_b = ((ha - patch) // 2, (wa - patch) // 2), ((hb - patch) // 2, (wb - patch) // 2)
    eye = np.eye(3)
    c = {
        # the destination patch IS the source patch; windows flush with the top-left corner
        "identity_tl": dict(image=0, inv_h=eye, win_src=(0, 0), win_dst=(0, 0), labels=("uniform", 60), exact=True),
        # flush with the bottom-right corner; points on the last column and the last row; fewer rows than the cut
        "identity_br": dict(image=1, inv_h=eye, win_src=(hb - patch, wb - patch), win_dst=(hb - patch, wb - patch),
                            labels=("edges", 12), exact=True),
        # dst(x, y) = src(x - 20, y + 7): the window flush with the left edge has 20 zero columns; flush with the bottom, 7 zero rows
        "shift_int": dict(image=0, inv_h=_shift(20.0, -7.0), win_src=mid_a, win_dst=(ha - patch, 0), labels=("uniform", 50), exact=True),
        "mild": dict(image=0, inv_h=MILD, win_src=(0, wa - patch), win_dst=(mid_a[0] + 3, mid_a[1] - 5), labels=("uniform", 80), exact=False),
        # the deliberate tie at the top_k cut
        "mild_tie": dict(image=1, inv_h=MILD, win_src=mid_b, win_dst=mid_b, labels=("tie", 40), exact=False),
        # minification: the destination samples the source two pixels apart
        "rot25_half": dict(image=1, inv_h=_rot(hb, wb, 25.0, 0.5), win_src=(0, wb - patch), win_dst=mid_b,
                           labels=("uniform", 70), exact=False),
        # the window samples entirely outside the source: an all-zero patch, dst_max == 0; every label warps outside
        "outside": dict(image=0, inv_h=_shift(1000.0, 1000.0), win_src=(ha - patch, 0), win_dst=mid_a, labels=("uniform", 30), exact=True),
        "no_labels": dict(image=1, inv_h=MILD, win_src=(0, 0), win_dst=(hb - patch, 0), labels=("uniform", 0), exact=False),
        "one_label": dict(image=0, inv_h=MILD, win_src=mid_a, win_dst=mid_a, labels=("centre", 1), exact=False),
        # duplicates after truncation; points inside the image but outside both windows
        "dups": dict(image=1, inv_h=np.array([[0.97, -0.02, 2.4], [0.03, 1.02, -1.7], [-3e-5, 5e-5, 1.0]]), win_src=mid_b,
                     win_dst=mid_b, labels=("dups", 24), exact=False),
        # fy == 0 in every row (an integer row shift) with fx == 24: dst(x, y) = src(x - 0.25, y - 3)
        "frac_x": dict(image=0, inv_h=_shift(0.25, 3.0), win_src=mid_a, win_dst=(0, 0), labels=("uniform", 20), exact=False),
        # fx == 0 in every column with fy == 24: dst(x, y) = src(x - 2, y - 0.25)
        "quarter_y": dict(image=1, inv_h=_shift(2.0, 0.25), win_src=mid_b, win_dst=(0, 0), labels=("uniform", 20), exact=False),
        # dst(x, y) = src(x + 0.25, y): in the last column the sx + 1 tap is outside the image (window flush right)
        "last_col": dict(image=0, inv_h=_shift(-0.25, 0.0), win_src=mid_a, win_dst=(mid_a[0], wa - patch), labels=("uniform", 16), exact=False),
    }
    return c


def batch_names(patch, p):
    names = list(cases(patch))
    return [names[i % len(names)] for i in range(p)]


def make_labels(kind, n, shape, seed):
    """[n,3] float32 rows (x, y, prob) inside an image of ``shape`` (h, w)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), rng.permutation(n) / max(n, 1) + 0.001], axis=1)
    if kind == "centre":
        pts[:, :2] = (w / 2 + 0.3, h / 2 + 0.6)
    if kind == "edges":
        pts[0, :2], pts[1, :2], pts[2, :2] = (w - 1, 0.4 * h), (0.3 * w, h - 1), (w - 1, h - 1)
        pts[3, :2] = (0, 0)
    if kind == "tie":                                             # five rows share the prob at the cut of TOP_KS[0]; three of them fit
        order = np.argsort(-pts[:, 2])
        pts[order[22:27], 2] = pts[order[22], 2]
    if kind == "dups":                                            # rows 0..7: four truncated pixels twice; the rest on the image's frame
        pts[0:4, :2] = np.array([w // 2, h // 2]) + np.array([(-5, 4), (3, -6), (7, 2), (-9, 8)]) + rng.uniform(0.05, 0.95, (4, 2))
        pts[4:8, :2] = np.floor(pts[0:4, :2]) + rng.uniform(0.05, 0.95, (4, 2))
        pts[8:16, 0], pts[16:24, 1] = rng.uniform(0, 3, 8), rng.uniform(0, 3, 8)
    return pts.astype(np.float32)


# ---- the image warp -------------------------------------------------------------------------------------------------------
def invert3(m):
    """common_mask.h's closed-form inverse, every product and sum rounded on its own."""
    a, b, c, d, e, f, g, h, i = (np.float64(v) for v in np.asarray(m, np.float64).reshape(9))
    A, B, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * B + c * C
    if det == 0.0:
        return None
    r = 1.0 / det
    return np.array([A * r, -(b * i - c * h) * r, (b * f - c * e) * r, B * r, (a * i - c * g) * r, -(a * f - c * d) * r,
                     C * r, -(a * h - b * g) * r, (a * e - b * d) * r])


def source_q5(m, ys, xs):
    """warp_source_q5 for arrays of output pixels -> (sx, sy, fx, fy) int64."""
    xs, ys = xs.astype(np.float64), ys.astype(np.float64)
    X0 = m[0] * xs + m[1] * ys + m[2]
    Y0 = m[3] * xs + m[4] * ys + m[5]
    W = m[6] * xs + m[7] * ys + m[8]
    with np.errstate(divide="ignore"):
        W = np.where(W != 0.0, 32.0 / W, 0.0)
    X = np.rint(np.clip(X0 * W, -2147483648.0, 2147483647.0)).astype(np.int64)
    Y = np.rint(np.clip(Y0 * W, -2147483648.0, 2147483647.0)).astype(np.int64)
    return X >> 5, Y >> 5, X & 31, Y & 31


def warp_perspective_u8(src, inv_h):
    """cv2.warpPerspective(src, inv_h, (w, h)) for a uint8 [H,W,3] image as include/balf_hip.h defines it: the whole image."""
    h, w = src.shape[:2]
    m = invert3(inv_h)
    if m is None:
        return np.zeros_like(src)
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy, fx, fy = source_q5(m, ys, xs)
    s = src.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok[..., None], s[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    assert ((w00 + w01 + w10 + w11) == 32768).all()
    total = tap(sy, sx) * w00[..., None] + tap(sy, sx + 1) * w01[..., None] + tap(sy + 1, sx) * w10[..., None] + \
        tap(sy + 1, sx + 1) * w11[..., None]
    return ((total + 16384) >> 15).astype(np.uint8)


def norm255(u8):
    """The reference's ``img / 255.0`` (float64) narrowed by ``torch.tensor(..., dtype=torch.float32)``."""
    return (u8.astype(np.float64) / 255.0).astype(np.float32)


def crop(a, win, patch):
    return a[win[0]:win[0] + patch, win[1]:win[1] + patch]


# ---- the labels -----------------------------------------------------------------------------------------------------------
def select_k_best(pts, k):
    """Row indices kept, ascending: the k rows of largest prob, ties at the cut: the lower row index."""
    if k == 0 or len(pts) <= k:
        return np.arange(len(pts))
    return np.sort(np.argsort(-pts[:, 2], kind="stable")[:k])


def warp_labels_f32(xy_int, inv_h):
    """Integer (x, y) rows through inv_h narrowed to float32, float32 arithmetic, (h0 x + h1 y) + h2 -> float32 (x', y')."""
    hm = np.asarray(inv_h, np.float64).astype(np.float32).reshape(9)
    x, y = xy_int[:, 0].astype(np.float32), xy_int[:, 1].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        zn = (hm[6] * x + hm[7] * y) + hm[8]
        return np.stack([((hm[0] * x + hm[1] * y) + hm[2]) / zn, ((hm[3] * x + hm[4] * y) + hm[5]) / zn], axis=1)


def heatmaps(pts, top_k, shape, inv_h):
    """-> (source heat map, destination heat map), float32 [H,W] of the FULL image."""
    h, w = shape
    kept = pts[select_k_best(pts, top_k)]
    xy = kept[:, :2].astype(np.int64)                            # truncation
    src, dst = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    ok = (xy[:, 0] >= 0) & (xy[:, 0] < w) & (xy[:, 1] >= 0) & (xy[:, 1] < h)
    src[xy[ok, 1], xy[ok, 0]] = 1.0
    wp = warp_labels_f32(xy, inv_h)
    ok = (wp[:, 0] >= 0) & (wp[:, 0] <= np.float32(w - 1)) & (wp[:, 1] >= 0) & (wp[:, 1] <= np.float32(h - 1))
    r = np.rint(wp[ok]).astype(np.int64)                         # half to even
    dst[r[:, 1], r[:, 0]] = 1.0
    return src, dst


# ---- one pair, whole ------------------------------------------------------------------------------------------------------
def pair_np(image, pts, top_k, inv_h, win_src, win_dst, patch):
    """What balf_synth_pairs computes for one pair, the reference's way: full arrays, then the crops.
    -> (img_src [3,p,p], img_dst [3,p,p], heat_src [1,p,p], heat_dst [1,p,p] float32, dst_max int)."""
    warped = crop(warp_perspective_u8(image, inv_h), win_dst, patch)
    hs, hd = heatmaps(pts, top_k, image.shape[:2], inv_h)
    return (np.ascontiguousarray(norm255(crop(image, win_src, patch)).transpose(2, 0, 1)),
            np.ascontiguousarray(norm255(warped).transpose(2, 0, 1)), crop(hs, win_src, patch)[None].copy(),
            crop(hd, win_dst, patch)[None].copy(), int(warped.max()))


def expected_from(patch, name, top_k, g):
    """The restatement's outputs of one case with the label rows of the fixture dict ``g``."""
    c = cases(patch)[name]
    return pair_np(images()[c["image"]], g[f"labels.{name}"], top_k, c["inv_h"], c["win_src"], c["win_dst"], patch)


@functools.lru_cache(maxsize=None)
def _expected(patch, name, top_k):
    return expected_from(patch, name, top_k, fixture())


def window_taps(patch, name):
    """(sx, sy, fx, fy) of the destination window's pixels of one case, [patch,patch] each."""
    c = cases(patch)[name]
    ys, xs = np.mgrid[c["win_dst"][0]:c["win_dst"][0] + patch, c["win_dst"][1]:c["win_dst"][1] + patch]
    return source_q5(invert3(c["inv_h"]), ys, xs)


def expected(patch, name, top_k):
    """The restatement's outputs of one case (computed once per process; callers must not write them)."""
    return _expected(patch, name, top_k)


def pack_batch(patch, names, labels):
    """The host arrays of one balf_synth_pairs call for the named cases, ``labels`` a mapping case name -> rows: -> dict of
    NumPy arrays (packed, offsets, sizes, inv_h, win_src, win_dst, pts, pts_offsets)."""
    ims = images()
    nbytes = [im.size for im in ims]
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    cs = [cases(patch)[n] for n in names]
    rows = [np.asarray(labels[n], np.float32).reshape(-1, 3) for n in names]
    return {"packed": np.concatenate([im.reshape(-1) for im in ims]),
            "offsets": np.asarray([starts[c["image"]] for c in cs], np.int64),
            "sizes": np.asarray([IMAGE_SHAPES[c["image"]] for c in cs], np.int32),
            "inv_h": np.stack([np.asarray(c["inv_h"], np.float64) for c in cs]),
            "win_src": np.asarray([c["win_src"] for c in cs], np.int32), "win_dst": np.asarray([c["win_dst"] for c in cs], np.int32),
            "pts": np.concatenate(rows) if rows else np.zeros((0, 3), np.float32),
            "pts_offsets": np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)}
