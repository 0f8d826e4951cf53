"""Shared by the resize-protocol tests (test_resize_repeat_host.py, test_resize_repeat_gpu.py) and the recording script
(tests/golden/make_resize_golden.py): access to tests/golden/resize_repeat.npz, a float64 NumPy restatement of
compute_resize_repeatability with the port's tie rule (higher prob first, then the lower row index), the integer NumPy
restatement of balf_resize_crop_u8's definition (include/balf_hip.h), and a synthetic HSequences-style loader."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_repeat.npz")
KEYS = ('repeatability', 'localization_err', 'common_src_num', 'common_dst_num', 'rep_src_num', 'rep_dst_num')


def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def case_names(g):
    return [str(n) for n in g["meta.cases"]]


def case_inputs(g, name):
    """-> (src rows [n,3], dst rows [m,3] (row, col, prob; fresh copies), h, shape_src, shape_dst, k, thresh)."""
    s = str(g[f"{name}.set"])
    src = g[f"rows.{s}.src"][:int(g[f"{name}.n_src"])].copy()
    dst = g[f"rows.{s}.dst"][:int(g[f"{name}.n_dst"])].copy()
    return (src, dst, g[f"{name}.h"].copy(), tuple(int(v) for v in g[f"{name}.shape_src"]),
            tuple(int(v) for v in g[f"{name}.shape_dst"]), int(g[f"{name}.k"]), float(g[f"{name}.thresh"]))


# ---- the metric -----------------------------------------------------------------------------------------------------------
def warp_cols_rows(col, row, m):
    """(x, y) = (col, row) through the 3x3 `m`, every product and sum rounded on its own (NumPy does not fuse)."""
    den = m[2, 0] * col + m[2, 1] * row + m[2, 2]
    nx = m[0, 0] * col + m[0, 1] * row + m[0, 2]
    ny = m[1, 0] * col + m[1, 1] * row + m[1, 2]
    return nx / den, ny / den


def select_k_best(rows, k):
    """The k rows of highest prob, ties: the lower row index; kept in their original order."""
    if len(rows) <= k:
        return rows[:, :2]
    keep = np.sort(np.argsort(-rows[:, 2], kind="stable")[:k])
    return rows[keep, :2]


def kept_rows(keypoints, warped_keypoints, h, shape_src, shape_dst, k, h_inv=None):
    """The two kept lists (row, col): warped source rows inside shape_dst, unwarped destination rows whose warp is inside
    shape_src, each cut to the k best."""
    kp, wkp = np.asarray(keypoints, np.float64).reshape(-1, 3), np.asarray(warped_keypoints, np.float64).reshape(-1, 3)
    h = np.asarray(h, np.float64)
    h_inv = np.linalg.inv(h) if h_inv is None else np.asarray(h_inv, np.float64)
    wc, wr = warp_cols_rows(wkp[:, 1], wkp[:, 0], h_inv)
    dst = wkp[(wr >= 0) & (wr < shape_src[0]) & (wc >= 0) & (wc < shape_src[1])]
    wc, wr = warp_cols_rows(kp[:, 1], kp[:, 0], h)
    src = np.stack([wr, wc, kp[:, 2]], axis=1)[(wr >= 0) & (wr < shape_dst[0]) & (wc >= 0) & (wc < shape_dst[1])]
    return select_k_best(src, k), select_k_best(dst, k)


def resize_repeatability_np(keypoints, warped_keypoints, h, shape_src, shape_dst, keep_k_points=1000, distance_thresh=5,
                            h_inv=None):
    """compute_resize_repeatability restated (float64): does not write its inputs.  Also returns the two minima arrays."""
    a, b = kept_rows(keypoints, warped_keypoints, h, shape_src, shape_dst, keep_k_points, h_inv)
    n1, n2 = len(a), len(b)
    dy, dx = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    d2 = dy * dy + dx * dx
    min1 = np.sqrt(d2.min(axis=1)) if n2 else np.zeros(0)
    min2 = np.sqrt(d2.min(axis=0)) if n1 else np.zeros(0)
    e1, e2 = min1[min1 <= distance_thresh], min2[min2 <= distance_thresh]
    c1, c2 = len(e1), len(e2)
    rep, err = 0.0, -1.0
    if c1 + c2 > 0:
        rep = (c1 + c2) / (n1 + n2) * 100.0
        err = e1.sum() / (c1 + c2) + e2.sum() / (c1 + c2)
    return {'repeatability': rep, 'localization_err': err, 'common_src_num': n1, 'common_dst_num': n2, 'rep_src_num': c1,
            'rep_dst_num': c2}, min1, min2


def tie_case(seed=5):
    """Rows whose prob takes a handful of values only: many ties at the keep_k_points cut on both sides."""
    rng = np.random.default_rng(seed)
    h = np.array([[1.01, 0.02, -3.0], [-0.015, 0.99, 2.0], [2e-5, -1e-5, 1.0]])
    src = np.stack([rng.uniform(0, 240, 900), rng.uniform(0, 320, 900), rng.integers(1, 6, 900) / 8.0], axis=1)
    wc, wr = warp_cols_rows(src[:, 1], src[:, 0], h)
    dst = np.stack([wr + rng.normal(0, 1.5, 900), wc + rng.normal(0, 1.5, 900), rng.integers(1, 6, 900) / 8.0], axis=1)
    return src, dst, h, (240, 320), (240, 320), 300, 3.0


# ---- the resize -----------------------------------------------------------------------------------------------------------
def resize_geometry(h, w, th, tw):
    """-> (new_h, new_w, top, left): np.round is half to even; the reference's four CropAndPad amounts in imgaug's order
    (top, right, bottom, left) make `top = hp` and `left = tw - new_w - wp`."""
    scale = max(th / h, tw / w)
    new_h, new_w = (int(v) for v in np.round(np.array([h, w]) * scale))
    hp, wp = (th - new_h) // 2, (tw - new_w) // 2
    return new_h, new_w, hp, tw - new_w - wp


def linear_taps(n_src, n_new):
    d = np.arange(n_new, dtype=np.float64)
    f = ((d + 0.5) * (np.float64(n_src) / np.float64(n_new)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= n_src - 1
    s = np.where(low, 0, np.where(high, n_src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), w0, w1


def ratio_preserving_resize_np(img, target_size):
    """Integer restatement of balf_resize_crop_u8 for one uint8 image [H,W] / [H,W,C]."""
    img = np.asarray(img)
    th, tw = int(target_size[0]), int(target_size[1])
    h, w = img.shape[:2]
    new_h, new_w, top, left = resize_geometry(h, w, th, tw)
    x0, x1, a0, a1 = linear_taps(w, new_w)
    y0, y1, b0, b1 = linear_taps(h, new_h)
    p = img.astype(np.int64).reshape(h, w, -1)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    s0 = p[y0][:, x0] * a0 + p[y0][:, x1] * a1
    s1 = p[y1][:, x0] * a0 + p[y1][:, x1] * a1
    v = (((b0[:, None, None] * (s0 >> 4)) >> 16) + ((b1[:, None, None] * (s1 >> 4)) >> 16) + 2) >> 2
    res = np.clip(v, 0, 255).astype(np.uint8)
    out = np.zeros((th, tw, p.shape[2]), np.uint8)
    ys, xs = np.arange(th) - top, np.arange(tw) - left
    oky, okx = (ys >= 0) & (ys < new_h), (xs >= 0) & (xs < new_w)
    out[np.ix_(oky, okx)] = res[np.ix_(ys[oky], xs[okx])]
    return out.reshape((th, tw) + img.shape[2:])


# ---- a synthetic loader ---------------------------------------------------------------------------------------------------
def warp_u8(src_u8, h_src_2_dst, hd, wd):
    """The destination image [hd,wd(,C)]: the source resampled (bilinear, 0 outside) at inv(h_src_2_dst) (x, y, 1)."""
    m = np.linalg.inv(h_src_2_dst)
    ys, xs = np.mgrid[0:hd, 0:wd].astype(np.float64)
    sx, sy = warp_cols_rows(xs, ys, m)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = sx - x0, sy - y0
    s = src_u8.astype(np.float64).reshape(src_u8.shape[0], src_u8.shape[1], -1)
    sh, sw = s.shape[:2]

    def at(yy, xx):
        ok = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        return np.where(ok[..., None], s[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)

    v = (at(y0, x0) * ((1 - ax) * (1 - ay))[..., None] + at(y0, x0 + 1) * (ax * (1 - ay))[..., None] +
         at(y0 + 1, x0) * ((1 - ax) * ay)[..., None] + at(y0 + 1, x0 + 1) * (ax * ay)[..., None])
    return np.clip(np.rint(v), 0, 255).astype(np.uint8).reshape((hd, wd) + src_u8.shape[2:])


def scaled_homography(i, src_hw, dst_hw):
    """Source -> destination: a mild perspective map in the source frame followed by the change of size."""
    (hs, ws), (hd, wd) = src_hw, dst_hw
    base = np.array([[1.0 + 0.01 * (i % 3), 0.02 * ((i % 5) - 2), 3.0 * ((i % 4) - 1.5)],
                     [-0.015 * ((i % 3) - 1), 1.0 - 0.01 * (i % 2), -2.0 * ((i % 3) - 1)],
                     [2e-5 * ((i % 5) - 2), -1e-5 * (i % 3), 1.0]])
    return np.diag([wd / ws, hd / hs, 1.0]) @ base


class SyntheticSequences:
    """``.sequences`` / ``get_sequence_data(i)`` as Resize_HSequences with resize_image=False: one synthetic scene per
    sequence, destinations warped by known homographies, images of several sizes; ``color`` makes 3-channel "BGR" images whose
    channels differ."""
    SIZES = ((300, 400), (480, 640), (333, 517), (600, 450))
    DST_SIZES = ((300, 400), (360, 480), (405, 539))

    def __init__(self, n_sequences=3, n_dst=2, color=False, seed=900):
        from balf_amd.utils import synth
        self.sequences = [f"v_synthetic_{i}" for i in range(n_sequences)]
        self.data = []
        for i in range(n_sequences):
            hs, ws = self.SIZES[i % len(self.SIZES)]
            src = synth.synthetic_gray_u8(hs, ws, seed + i)
            if color:
                src = np.stack([src, 255 - src, (src.astype(np.int64) * 2 // 3).astype(np.uint8)], axis=2)
            dsts, hs_ = [], []
            for k in range(n_dst):
                hd, wd = self.DST_SIZES[(i + k) % len(self.DST_SIZES)]
                h = scaled_homography(i + 2 * k, (hs, ws), (hd, wd))
                dsts.append(warp_u8(src, h, hd, wd))
                hs_.append(h)
            self.data.append({'im_src_BGR': src, 'images_dst_BGR': dsts, 'homographies': np.asarray(hs_),
                              'sequence_name': self.sequences[i]})

    def get_sequence_data(self, i):
        return self.data[i]
