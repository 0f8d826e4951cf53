"""Shared by tests/test_training_input_edges_host.py and tests/test_training_input_edges_gpu.py: the case
builders that take balf_synth_pairs and balf_detector_loss past one workgroup's stride, and the CPU properties those cases
rely on.  Nothing here restates an operation: the references are tests/pair_synth_common.py (pair_np, warp_perspective_u8,
heatmaps, select_k_best) and tests/detector_loss_common.py (restate64).  pack_pairs is pair_synth_common.pack_batch without
its tie to the two fixture images: data layout only.

A pair is a dict(name, image (index into the call's images), inv_h, win_src, win_dst (top, left), pts [n,3] float32); a call
is a dict(images, pairs, top_k, patch).  The builders are seeded and cached; callers must not write what they return."""
import functools

import numpy as np
import torch

from tests import detector_loss_common as D
from tests import pair_synth_common as S

IMG_THREADS, IMG_PX, LBL_THREADS = 256, 4, 1024          # pair_synth.hip: kImgThreads, kImgPx, kLblThreads
LOSS_THREADS, LOSS_WAVE = 256, 64                        # detector_loss.hip: kLossThreads, the lanes of wave_sum_partials


# ---- the general packer ---------------------------------------------------------------------------------------------------
def pack_pairs(images, pairs):
    """The host arrays of one balf_synth_pairs call: every image of ``images`` (uint8 [H,W,3]) back to back in order, whether
    a pair uses it or not, as pack_batch lays them out -> dict of NumPy arrays (packed, offsets, sizes, inv_h, win_src, win_dst,
    pts, pts_offsets)."""
    starts = np.concatenate([[0], np.cumsum([im.size for im in images])[:-1]])
    rows = [np.asarray(p["pts"], np.float32).reshape(-1, 3) for p in pairs]
    return {"packed": np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]),
            "offsets": np.asarray([starts[p["image"]] for p in pairs], np.int64),
            "sizes": np.asarray([images[p["image"]].shape[:2] for p in pairs], np.int32),
            "inv_h": np.stack([np.asarray(p["inv_h"], np.float64).reshape(3, 3) for p in pairs]),
            "win_src": np.asarray([p["win_src"] for p in pairs], np.int32),
            "win_dst": np.asarray([p["win_dst"] for p in pairs], np.int32),
            "pts": np.concatenate(rows),
            "pts_offsets": np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)}


def pack_call(call):
    return pack_pairs(call["images"], call["pairs"])


def expected_pair(call, i):
    """The restatement's (img_src, img_dst, heat_src, heat_dst, dst_max) of pair i of a call."""
    p = call["pairs"][i]
    return S.pair_np(call["images"][p["image"]], p["pts"], call["top_k"], p["inv_h"], p["win_src"], p["win_dst"], call["patch"])


def single(call, i):
    """Pair i of a call as a call of its own (same images, so the same offsets)."""
    return {**call, "pairs": [call["pairs"][i]]}


def _pair(name, image, inv_h, win_src, win_dst, pts):
    return dict(name=name, image=image, inv_h=np.asarray(inv_h, np.float64), win_src=tuple(int(v) for v in win_src),
                win_dst=tuple(int(v) for v in win_dst), pts=np.asarray(pts, np.float32).reshape(-1, 3))


def _random_rgb(h, w, seed, low=1, high=256):
    return np.random.default_rng(seed).integers(low, high, (h, w, 3), dtype=np.uint8)


# ---- A. nblk on and past 1024 ---------------------------------------------------------------------------------------------
BIG_PATCHES = (1024, 1028)
BIG_NBLK = {1024: 1024, 1028: 1033}
DIM, BRIGHT = 100, 255


def image_blocks(patch):
    """The image kernel's workgroups per side and pair (pair_synth.hip: image_blocks)."""
    quads = ((patch + IMG_PX - 1) // IMG_PX) * patch
    return (quads + IMG_THREADS - 1) // IMG_THREADS


def bright_at(patch):
    """(row, column, channel) of the single bright byte: the LAST row of the patch, in the last workgroup's quads."""
    return patch - 1, patch - 3, 1


@functools.lru_cache(maxsize=None)
def big_patch_call(patch):
    """Two pairs of a patch x patch image under the identity, the window the whole image: every byte <= DIM, the first pair's
    image with one BRIGHT byte in its last row; the second pair's image is the same without it."""
    dim = _random_rgb(patch, patch, 900 + patch, 0, DIM + 1)
    bright = dim.copy()
    bright[bright_at(patch)] = BRIGHT
    pts = [S.make_labels("edges", 40, (patch, patch), 910 + patch), S.make_labels("uniform", 33, (patch, patch), 911 + patch)]
    pairs = [_pair(n, i, np.eye(3), (0, 0), (0, 0), pts[i]) for i, n in enumerate(("bright", "dim"))]
    return dict(images=[bright, dim], pairs=pairs, top_k=25, patch=patch)


# ---- A. more label rows than threads, wide ties -----------------------------------------------------------------------------
ROWS_PATCH = 128
ROW_COUNTS = (1023, 1024, 1025, 5000)
ROW_TOP_KS = tuple(sorted({0, 1} | {n + d for n in ROW_COUNTS for d in (-1, 0, 1)} | {n // 2 for n in ROW_COUNTS}))
TIE_TOP_K = 1500


@functools.lru_cache(maxsize=None)
def rows_images():
    return [_random_rgb(200, 264, 920), _random_rgb(192, 256, 921)]


def unique_pixel_rows(n, win, probs, seed):
    """n rows (x, y, prob) whose truncated pixels are n DIFFERENT pixels of the ROWS_PATCH window at ``win``: the source heat
    map then holds exactly one 1.0 per kept row, so that a wrong selection of a single row shows."""
    rng = np.random.default_rng(seed)
    pix = rng.permutation(ROWS_PATCH * ROWS_PATCH)[:n]
    xy = np.stack([win[1] + pix % ROWS_PATCH + 0.25, win[0] + pix // ROWS_PATCH + 0.5], axis=1)
    return np.concatenate([xy, np.asarray(probs, np.float64).reshape(n, 1)], axis=1).astype(np.float32)


def _rows_geometry():
    """(image, inv_h, win_src, win_dst) of the four pairs of the label-row calls."""
    (ha, wa), (hb, wb) = (im.shape[:2] for im in rows_images())
    p = ROWS_PATCH
    return ((0, np.eye(3), (7, 11), (7, 11)),
            (1, S.MILD, (hb - p, wb - p), ((hb - p) // 2, (wb - p) // 2)),
            (0, S._shift(20.0, -7.0), ((ha - p) // 2, (wa - p) // 2), (ha - p, 0)),
            (1, S._rot(hb, wb, 25.0, 0.5), (0, wb - p), ((hb - p) // 2, (wb - p) // 2)),
            (0, S.MILD, (ha - p, 3), ((ha - p) // 2, (wa - p) // 2)))


@functools.lru_cache(maxsize=None)
def _many_rows_pairs():
    pairs = []
    for i, (n, (image, inv_h, ws, wd)) in enumerate(zip(ROW_COUNTS, _rows_geometry())):
        probs = np.random.default_rng(930 + i).permutation(n) / n + 0.001                # all different in float32
        pairs.append(_pair(f"n{n}", image, inv_h, ws, wd, unique_pixel_rows(n, ws, probs, 940 + i)))
    return pairs


def many_rows_call(top_k):
    """1023, 1024, 1025 and 5000 rows in ONE call: pts_offsets carries across the pairs."""
    return dict(images=rows_images(), pairs=_many_rows_pairs(), top_k=top_k, patch=ROWS_PATCH)


TIE_GROUP = 100 + 117 * np.arange(40)                    # row indices of the 40 tied rows of "spread_tie"
TIE_ABOVE = 1483                                         # rows of "spread_tie" above the tied prob: 17 of the group fit


@functools.lru_cache(maxsize=None)
def wide_tie_call():
    """Five pairs cut at TIE_TOP_K = 1500, name -> what the second select must do:
    all_equal    5000 equal probs: rows 0..1499
    spread_tie   5000 rows, 1483 above a group of 40 tied rows 117 indices apart: the group's first 17
    zeros_neg_first / zeros_pos_first   3000 rows, 1490 positive, 1490 negative, 20 zeros of which the 10 of lower index are -0.0
                 (+0.0): the cut falls between the two signs of zero, which compare equal: the 10 of lower index
    negative     4000 different negative probs."""
    geo = _rows_geometry()
    rng = np.random.default_rng(950)
    probs = {"all_equal": np.full(5000, 0.25)}
    spread = np.empty(5000)
    others = np.setdiff1d(np.arange(5000), TIE_GROUP)
    others = others[rng.permutation(len(others))]
    spread[TIE_GROUP] = 0.5
    spread[others[:TIE_ABOVE]] = 0.5 + (1 + np.arange(TIE_ABOVE)) / 4000.0
    spread[others[TIE_ABOVE:]] = 0.5 - (1 + np.arange(len(others) - TIE_ABOVE)) / 8000.0
    probs["spread_tie"] = spread
    order = rng.permutation(3000)
    zeros = np.sort(order[2980:])
    for name, low in (("zeros_neg_first", -0.0), ("zeros_pos_first", 0.0)):
        v = np.empty(3000)
        v[order[:1490]] = (1 + np.arange(1490)) / 2000.0
        v[order[1490:2980]] = -(1 + np.arange(1490)) / 2000.0
        v[zeros[:10]], v[zeros[10:]] = low, -low
        probs[name] = v
    probs["negative"] = -(1 + rng.permutation(4000)) / 4000.0
    pairs = [_pair(name, image, inv_h, ws, wd, unique_pixel_rows(len(probs[name]), ws, probs[name], 960 + i))
             for i, (name, (image, inv_h, ws, wd)) in enumerate(zip(probs, geo))]
    return dict(images=rows_images(), pairs=pairs, top_k=TIE_TOP_K, patch=ROWS_PATCH)


def wide_tie_kept():
    """name -> the row indices the documented rule keeps (higher prob first, then the lower row index), written down from how
    wide_tie_call builds its probs, not computed by a selection."""
    c = {p["name"]: p["pts"][:, 2] for p in wide_tie_call()["pairs"]}
    zeros = {n: np.flatnonzero(c[n] == 0.0) for n in ("zeros_neg_first", "zeros_pos_first")}
    return {"all_equal": np.arange(TIE_TOP_K),
            "spread_tie": np.sort(np.concatenate([np.flatnonzero(c["spread_tie"] > np.float32(0.5)), TIE_GROUP[:17]])),
            "zeros_neg_first": np.sort(np.concatenate([np.flatnonzero(c["zeros_neg_first"] > 0.0), zeros["zeros_neg_first"][:10]])),
            "zeros_pos_first": np.sort(np.concatenate([np.flatnonzero(c["zeros_pos_first"] > 0.0), zeros["zeros_pos_first"][:10]])),
            "negative": np.flatnonzero(c["negative"] > np.float32(-(TIE_TOP_K + 0.5) / 4000.0))}


# ---- A. label geometry, the pole of the image warp, singular inv_h ----------------------------------------------------------
EDGE_SHAPES = ((96, 128), (80, 112))
POLE_COLUMN = 64
POLE_TILT = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def edge_images():
    """Two RGB images without a zero byte: a pixel that samples inside the image is never 0."""
    return [_random_rgb(h, w, 970 + i) for i, (h, w) in enumerate(EDGE_SHAPES)]


def pole_matrix(tilt):
    """inv_h = [[1,0,0],[0,1,0],[1/64,tilt,1]]: its closed-form inverse is exactly [[1,0,0],[0,1,0],[-1/64,-tilt,1]], so the
    image warp's W = 1 - x / 64 - tilt * y.  tilt = 0: W == 0 in all of column 64.  tilt = +-2^-40: W == 0 at (64, 0) and
    -+y * 2^-40 in the rest of the column: 32 / W times x = 64 saturates the clamp at -2^31 (+2^31 - 1)."""
    return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0 / POLE_COLUMN, tilt, 1.0]])


ZN_ZERO = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 16.0, 0.0, 1.0]])      # the label warp's zn == 0 at x = 16
HALF_SHIFT = S._shift(2.5, 3.5)                                                       # integer labels land on .5
MAX_SHIFT = S._shift(5.0, 3.0)
SINGULAR = {"zero_row": np.array([[1.0, 0.1, 2.0], [0.0, 0.0, 0.0], [1e-4, 0.0, 1.0]]),
            "rank_one": np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])}


@functools.lru_cache(maxsize=None)
def edge_pairs(patch):
    """The pairs of the label-geometry, pole and singular edges for one patch size, on edge_images(); the singular pairs
    stand between ordinary ones.  Every pair also carries some uniform rows."""
    (ha, wa), (hb, wb) = EDGE_SHAPES
    mid_a, mid_b = ((ha - patch) // 2, (wa - patch) // 2), ((hb - patch) // 2, (wb - patch) // 2)
    shapes = EDGE_SHAPES

    def rows(image, seed, special=()):
        uniform = S.make_labels("uniform", 30, shapes[image], seed)
        if not len(special):
            return uniform
        sp = np.asarray(special, np.float64)
        return np.concatenate([np.concatenate([sp, np.linspace(2.0, 3.0, len(sp))[:, None]], axis=1).astype(np.float32), uniform])

    trunc = [(-0.5, 3.3), (4.7, -0.9), (-0.99, -0.01), (-1.0, 5.0), (5.0, -1.0), (-1.5, 2.0), (wa - 0.5, 2.0), (float(wa), 2.0),
             (2.0, ha - 0.5), (2.0, float(ha)), (1.9, 1.9)]
    zn0 = [(float(x) + 0.3, 1.0 + (x % 5) + 0.6) for x in range(0, 22)]                 # x = 16 among them
    half = [(mid_b[1] + dx + 0.2, mid_b[0] + dy + 0.7) for dx in range(0, min(patch, 6)) for dy in range(0, min(patch, 6))]
    top_m, left_m = ha - patch - 3, wa - patch - 5
    # under MAX_SHIFT (x + 5, y + 3): on x_max only, on y_max only, on both, one past x_max, one past y_max, just inside
    on_max = [(wa - 6 + 0.3, ha - 5 + 0.2), (wa - 7 + 0.4, ha - 4 + 0.6), (wa - 6 + 0.5, ha - 4 + 0.5), (wa - 5 + 0.1, ha - 5 + 0.2),
              (wa - 7 + 0.5, ha - 3 + 0.3), (wa - 8 + 0.9, ha - 6 + 0.9)]
    far = [(1.5, 1.5), (wb - 1.2, 1.7), (1.1, hb - 1.3), (wb - 1.6, hb - 1.4), (wb / 2.0, 0.5)]
    pole_left = POLE_COLUMN - patch // 2
    pairs = [_pair("mild", 0, S.MILD, mid_a, (mid_a[0] + 3, mid_a[1] - 5), rows(0, 980)),
             _pair("zero_row", 0, SINGULAR["zero_row"], mid_a, (0, mid_a[1]), rows(0, 981)),      # (labels land on row 0)
             _pair("rot", 1, S._rot(hb, wb, 25.0, 0.5), (0, wb - patch), mid_b, rows(1, 982)),
             _pair("rank_one", 1, SINGULAR["rank_one"], mid_b, (0, 0), rows(1, 983, [(0.2, 0.4), (1.5, 0.5), (3.3, 2.2)])),
             _pair("trunc", 0, np.eye(3), (0, 0), (0, 0), rows(0, 984, trunc)),
             _pair("zn_zero", 0, ZN_ZERO, (0, 0), (0, 0), rows(0, 985, zn0)),
             _pair("half", 1, HALF_SHIFT, mid_b, mid_b, rows(1, 986, half)),
             _pair("on_max", 0, MAX_SHIFT, (top_m, left_m), (ha - patch, wa - patch), rows(0, 987, on_max)),
             _pair("far", 1, S.MILD, mid_b, mid_b, rows(1, 988, far)),
             _pair("pole", 0, pole_matrix(0.0), (0, 0), (0, pole_left), rows(0, 989)),
             _pair("pole_neg", 0, pole_matrix(POLE_TILT), (0, pole_left), (0, pole_left), rows(0, 990)),
             _pair("pole_pos", 0, pole_matrix(-POLE_TILT), mid_a, (0, pole_left), rows(0, 991))]
    return pairs


EDGE_PATCH = 32
TINY_PATCHES = (1, 2, 3, 5)


def edge_call(patch, top_k=0):
    return dict(images=edge_images(), pairs=edge_pairs(patch), top_k=top_k, patch=patch)


def edge_names():
    return [p["name"] for p in edge_pairs(EDGE_PATCH)]


MANY_PAIRS, MANY_PATCH, MANY_TOP_K = 64, 8, 25
MANY_SPOT = (1, 21, 40, 63)                              # zero_row, pole, a 1100-row pair, rank_one of the last cycle


@functools.lru_cache(maxsize=None)
def many_pairs_call():
    """64 pairs of patch 8 cycling edge_pairs(8); pairs 7 and 40 carry 1100 rows, so that later pairs' pts_offsets lie past
    one pass of the label kernel's threads."""
    base = edge_pairs(MANY_PATCH)
    pairs = [dict(base[i % len(base)]) for i in range(MANY_PAIRS)]
    for i in (7, 40):
        shape = EDGE_SHAPES[pairs[i]["image"]]
        pairs[i]["pts"] = np.concatenate([pairs[i]["pts"], S.make_labels("uniform", 1100 - len(pairs[i]["pts"]), shape, 995 + i)])
    return dict(images=edge_images(), pairs=pairs, top_k=MANY_TOP_K, patch=MANY_PATCH)


def pole_window_W(pair, patch):
    """W of warp_source_q5 and its 1/32-pixel X, Y (before the shift) over the destination window of a pole pair, float64 in
    the kernel's order of operations."""
    m = S.invert3(pair["inv_h"])
    top, left = pair["win_dst"]
    ys, xs = np.mgrid[top:top + patch, left:left + patch]
    W = m[6] * xs.astype(np.float64) + m[7] * ys.astype(np.float64) + m[8]
    sx, sy, fx, fy = S.source_q5(m, ys, xs)
    return W, sx * 32 + fx, sy * 32 + fy


# ---- B. the anchor loss past one wave of partials ---------------------------------------------------------------------------
# 16128, 16129, 16384 and 16510 cells: nblk = 63 (full), 64 (one cell in the last), 64 (full), 65
LOSS_PLANES = ((126, 128), (127, 127), (128, 128), (127, 130))
LOSS_THIN = ((1, 16641), (16641, 1))                     # nblk = 66
LOSS_WORKLOAD = (136, 240)                               # nblk = 128
LOSS_NBLK = {(126, 128): 63, (127, 127): 64, (128, 128): 64, (127, 130): 65, (1, 16641): 66, (16641, 1): 66, (136, 240): 128}
LATE_PLANE = (127, 130)
LATE_FIRST_CELL = LOSS_WAVE * LOSS_THREADS               # the first cell of workgroup 64


def loss_nblk(hc, wc):
    return (hc * wc + LOSS_THREADS - 1) // LOSS_THREADS


def loss_case(hc, wc, with_mask, b=3, last_masked=True):
    """Seeded inputs of one plane (detector_loss_common.make_case): with a mask and noise, or without both."""
    c = D.make_case((b, hc, wc), (300 if with_mask else 400) + hc * 100003 + wc, with_mask=with_mask, last_masked=last_masked)
    return c if with_mask else {**c, "noise": None}


def late_cells_case():
    """B = 2 on the 127 x 130 plane: image 0's mask is zero in every cell of workgroups 0..63 and one in the 126 cells of
    workgroup 64; image 1 keeps the drawn mask."""
    hc, wc = LATE_PLANE
    c = D.make_case((2, hc, wc), 77, last_masked=False)
    cells = (torch.arange(hc * wc) >= LATE_FIRST_CELL).float().reshape(hc, wc)
    c["valid_mask"][0, 0] = cells.repeat_interleave(8, dim=0).repeat_interleave(8, dim=1)
    return c


def valid_cells(valid_mask):
    """[B,1,8Hc,8Wc] -> bool [B, Hc*Wc]: the cells whose 64 pixels are all non-zero."""
    return (D.space_to_depth(valid_mask).prod(dim=1) != 0).reshape(valid_mask.shape[0], -1).numpy()
