"""What the NMS-score-map tests share (tests/test_nms_map_host.py, tests/test_nms_map_gpu.py, tests/golden/make_nms_map_golden.py):
a NumPy oracle of both protocols of balf_nms_score_map with the project's tie rule, the fixture's cases and its inputs.

Oracle: candidates = pixels >= the threshold, visited in the order of a STABLE sort by (-score, raster index); one is kept iff no
kept candidate has it inside its footprint; ``keep_top_k`` takes the first of the kept list, which is in that order already.  The
footprint of the box protocol is the set of offsets at which two size x size boxes have IoU > iou, with the float32 operations of
the reference's box_iou on two explicit boxes; the greedy protocol's is the full (2 d + 1)^2 square.
"""
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nms_map.npz")
CONF = 0.015                                    # min_prob / conf_thresh of the reference's defaults
BOX_ARGS = ((4, 0.1, -1), (4, 0.1, 50), (3, 0.3, -1), (8.5, 0.1, 7))      # (size, iou, keep_top_k) recorded per case
GREEDY_DISTS = (4, 15)
SYNTH_SHAPES = {"s40x72": (40, 72, 1), "s33x130": (33, 130, 2)}            # name -> (H, W, seed)
NATURAL_CROP = ("im1.prob", 40, 72)             # the key of tests/golden/natural.npz and the crop's size
CASES = tuple(SYNTH_SHAPES) + ("natural",)


def synthetic_scores(name):
    """A seeded permutation of H * W distinct float32 values in (0, 0.04): a little over a third of them below CONF."""
    h, w, seed = SYNTH_SHAPES[name]
    n = h * w
    v = ((np.arange(n, dtype=np.float64) + 1.0) / (n + 1.0) * 0.04).astype(np.float32)
    assert len(np.unique(v)) == n
    return v[np.random.RandomState(seed).permutation(n)].reshape(h, w)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def box_iou_f32(dr, dc, size, at=(100, 200)):
    """IoU of the box around ``at`` and the one around ``at + (dr, dc)``, float32 throughout as the reference's box_iou computes it
    on the float32 boxes (r - size/2, c - size/2, r + size/2, c + size/2)."""
    f = np.float32
    half = size / 2.0
    a = [f(at[0] - half), f(at[1] - half), f(at[0] + half), f(at[1] + half)]
    b = [f(at[0] + dr - half), f(at[1] + dc - half), f(at[0] + dr + half), f(at[1] + dc + half)]
    area_a = f(f(a[2] - a[0]) * f(a[3] - a[1]))
    area_b = f(f(b[2] - b[0]) * f(b[3] - b[1]))
    wh0 = max(f(min(a[2], b[2]) - max(a[0], b[0])), f(0))
    wh1 = max(f(min(a[3], b[3]) - max(a[1], b[1])), f(0))
    inter = f(wh0 * wh1)
    return f(inter / f(f(area_a + area_b) - inter))


def box_footprint_direct(size, iou, reach=None):
    """(radius, inside): inside[dr + reach, dc + reach] = IoU(dr, dc) > float32(iou), evaluated offset by offset out to ``reach``
    (default: radius = ceil(size) - 1)."""
    radius = int(np.ceil(size)) - 1
    reach = radius if reach is None else reach
    inside = np.zeros((2 * reach + 1, 2 * reach + 1), dtype=bool)
    for dr in range(-reach, reach + 1):
        for dc in range(-reach, reach + 1):
            inside[dr + reach, dc + reach] = box_iou_f32(dr, dc, size) > np.float32(iou)
    return radius, inside


def square_footprint(dist):
    return dist, np.ones((2 * dist + 1, 2 * dist + 1), dtype=bool)


def sweep(score, conf, footprint, keep_top_k=-1):
    """The sequential sweep -> (map, count)."""
    radius, inside = footprint
    score = np.asarray(score, dtype=np.float32)
    h, w = score.shape
    flat = score.ravel()
    cand = np.flatnonzero(flat >= np.float32(conf))
    order = cand[np.argsort(-flat[cand], kind="stable")]
    alive = np.zeros((h + 2 * radius, w + 2 * radius), dtype=bool)
    alive[radius:radius + h, radius:radius + w] = score >= np.float32(conf)
    free = ~inside
    kept = []
    for idx in order:
        y, x = divmod(int(idx), w)
        if alive[y + radius, x + radius]:
            kept.append(idx)
            alive[y:y + 2 * radius + 1, x:x + 2 * radius + 1] &= free
    if keep_top_k > 0:
        kept = kept[:keep_top_k]
    out = np.zeros_like(score)
    out.ravel()[kept] = flat[kept]
    return out, len(kept)


def box_oracle(score, size, iou, min_prob=CONF, keep_top_k=-1):
    return sweep(score, min_prob, box_footprint_direct(size, iou), keep_top_k)


def greedy_oracle(score, dist, conf=CONF):
    return sweep(score, conf, square_footprint(dist))


def box_key(size, iou, k):
    return f"box_s{size}_i{iou}_k{k}"


def fixture():
    return np.load(FIXTURE)


def fixture_cases(fx):
    """(case, score, label, expected map, call) for every recorded map; call = ("box", size, iou, k) or ("greedy", dist)."""
    out = []
    for case in CASES:
        score = fx[f"{case}.score"]
        for size, iou, k in BOX_ARGS:
            out.append((case, score, box_key(size, iou, k), fx[f"{case}.{box_key(size, iou, k)}"], ("box", size, iou, k)))
        for d in GREEDY_DISTS:
            out.append((case, score, f"greedy_d{d}", fx[f"{case}.greedy_d{d}"], ("greedy", d)))
    return out


def same_map(got, want):
    """Bit equality of two float32 maps (+0.0 and -0.0 differ, as do NaN payloads)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
