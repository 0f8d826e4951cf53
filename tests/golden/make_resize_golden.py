#!/usr/bin/env python3
"""Record tests/golden/resize_repeat.npz by running the REFERENCE's compute_resize_repeatability
(balf/benchmark_test/repeatability_tools.py) and adapt_homography_to_preprocessing (balf/datasets/dataset_utils.py) unchanged.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_resize_golden.py

Both modules import cv2 / imgaug (absent offline), so the two function bodies are compiled from the reference's source with
``ast`` and run as they are, as make_val_golden.py does; both need NumPy only.  The fixture holds numbers only.  The reference
function overwrites its ``keypoints`` argument with the warped coordinates, so it is handed COPIES.

Row sets are stored once and shared by the cases (a case = a row set, a prefix length per side, a homography, two shapes,
keep_k_points, distance_thresh), which keeps the file small.

CONDITIONS ON THE RECORDED INPUTS (asserted here; a failing seed is replaced by the next one -- a condition on inputs, nothing
is skipped at test time): no two rows tie in prob at the k-th cut of either side (the reference's choice there is NumPy's
unstable argsort); no warped coordinate within 1e-9 of a bound it is tested against; no minimum distance within 1e-9 of the
threshold."""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from tests.golden.make_golden import ref_functions                 # noqa: E402
from tests import resize_repeat_common as C                          # noqa: E402

REF = "/root/reference/balf/"
MARGIN = 1e-9

MILD = np.array([[1.015, 0.02, -4.0], [-0.02, 0.99, 3.5], [3e-5, -2e-5, 1.0]])
SHIFT = np.array([[1.0, 0.01, 295.0], [0.005, 1.0, 2.0], [0.0, 0.0, 1.0]])            # a strip about 25 pixels wide
GROW = np.diag([400 / 320.0, 300 / 240.0, 1.0]) @ MILD                                # 240x320 -> 300x400
FAR = np.array([[1.0, 0.0, 0.25], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]])

# (case, row set, rows used per side, homography, shape_src, shape_dst, keep_k_points, distance_thresh)
CASES = (("both_above_k", "a", 1500, 1500, MILD, (240, 320), (240, 320), 1000, 5),
         ("src_above_k", "a", 1500, 700, MILD, (240, 320), (240, 320), 1000, 3),
         ("dst_above_k", "a", 650, 1500, MILD, (240, 320), (240, 320), 1000, 1),
         ("neither_above_k", "a", 800, 700, MILD, (240, 320), (240, 320), 1000, 5),
         ("k300", "a", 1500, 1500, MILD, (240, 320), (240, 320), 300, 3),
         ("k300_thresh1", "a", 900, 1500, MILD, (240, 320), (240, 320), 300, 1),
         ("shift", "a", 1500, 1500, SHIFT, (240, 320), (240, 320), 1000, 5),
         ("unequal_shapes", "b", 1200, 1400, GROW, (240, 320), (300, 400), 1000, 3),
         ("empty_src", "a", 0, 500, MILD, (240, 320), (240, 320), 1000, 5),
         ("empty_dst", "a", 500, 0, MILD, (240, 320), (240, 320), 1000, 5),
         ("both_empty", "a", 0, 0, MILD, (240, 320), (240, 320), 1000, 5),
         ("none_within", "far", 6, 6, FAR, (240, 320), (240, 320), 1000, 1),
         ("integer_rows", "int", 1500, 1500, MILD, (240, 320), (240, 320), 1000, 3),
         ("integer_rows_k300", "int", 1500, 1200, MILD, (240, 320), (240, 320), 300, 5))


def row_set(name, seed):
    """-> (src [n,3], dst [n,3]) rows (row, col, prob).  Half of the destination rows are source rows carried through the set's
    homography with 1.5 pixels of noise (repeatable points), the rest are unrelated."""
    rng = np.random.default_rng([31, seed])
    if name == "far":                        # six points per side, every one more than 1 pixel from all others' images
        src = np.stack([rng.uniform(20, 100, 6), rng.uniform(20, 140, 6), rng.uniform(0.1, 1, 6)], axis=1)
        dst = np.stack([rng.uniform(130, 220, 6), rng.uniform(170, 300, 6), rng.uniform(0.1, 1, 6)], axis=1)
        return src, dst
    h, (hs, ws), (hd, wd) = (GROW, (240, 320), (300, 400)) if name == "b" else (MILD, (240, 320), (240, 320))
    n = 1500
    src = np.stack([rng.uniform(0, hs, n), rng.uniform(0, ws, n), rng.uniform(0.01, 1.0, n)], axis=1)
    wc, wr = C.warp_cols_rows(src[:, 1], src[:, 0], h)
    dst = np.stack([wr + rng.normal(0, 1.5, n), wc + rng.normal(0, 1.5, n), rng.uniform(0.01, 1.0, n)], axis=1)
    loose = rng.random(n) < 0.5
    dst[loose, 0], dst[loose, 1] = rng.uniform(0, hd, loose.sum()), rng.uniform(0, wd, loose.sum())
    order = rng.permutation(n)
    dst = dst[order]
    if name == "int":                        # what the detector produces: integer pixels, float32 scores
        src[:, :2], dst[:, :2] = np.floor(src[:, :2]), np.clip(np.rint(dst[:, :2]), 0, [hd - 1, wd - 1])
        src[:, 2], dst[:, 2] = src[:, 2].astype(np.float32), dst[:, 2].astype(np.float32)
    return src, dst


def conditions_hold(src, dst, h, shape_src, shape_dst, k, thresh):
    h_inv = np.linalg.inv(h)
    for rows, m, (hl, wl), warped_on in ((dst, h_inv, shape_src, False), (src, h, shape_dst, True)):
        wc, wr = C.warp_cols_rows(rows[:, 1], rows[:, 0], m)
        for v, lim in ((wr, hl), (wc, wl)):
            if len(v) and min(np.abs(v).min(), np.abs(v - lim).min()) < MARGIN:
                return False
        prob = rows[(wr >= 0) & (wr < hl) & (wc >= 0) & (wc < wl), 2]
        if len(prob) > k:
            s = np.sort(prob)[::-1]
            if s[k - 1] == s[k]:
                return False
    _, min1, min2 = C.resize_repeatability_np(src, dst, h, shape_src, shape_dst, k, thresh)
    return all(len(m) == 0 or np.abs(m - thresh).min() > MARGIN for m in (min1, min2))


def main():
    metric = ref_functions(REF + "benchmark_test/repeatability_tools.py", ["compute_resize_repeatability"])["compute_resize_repeatability"]
    adapt = ref_functions(REF + "datasets/dataset_utils.py", ["adapt_homography_to_preprocessing"])["adapt_homography_to_preprocessing"]
    fx = {"meta.cases": np.asarray([c[0] for c in CASES])}
    sets = {}
    for name in sorted({c[1] for c in CASES}):
        mine = [c for c in CASES if c[1] == name]
        for seed in range(20):
            src, dst = row_set(name, seed)
            if all(conditions_hold(src[:c[2]], dst[:c[3]], *c[4:]) for c in mine):
                break
            print(f"row set {name}: seed {seed} violates a condition, trying the next")
        else:
            raise AssertionError(name)
        sets[name] = (src, dst)
        fx[f"rows.{name}.src"], fx[f"rows.{name}.dst"] = src, dst
    for case, s, n_src, n_dst, h, shape_src, shape_dst, k, thresh in CASES:
        src, dst = sets[s][0][:n_src], sets[s][1][:n_dst]
        keep = src.copy()
        r = metric(src.copy(), dst.copy(), h.copy(), shape_src, shape_dst, keep_k_points=k, distance_thresh=thresh)
        assert np.array_equal(keep, src)
        fx[f"{case}.set"], fx[f"{case}.n_src"], fx[f"{case}.n_dst"], fx[f"{case}.h"] = np.asarray(s), n_src, n_dst, h
        fx[f"{case}.shape_src"], fx[f"{case}.shape_dst"] = np.asarray(shape_src), np.asarray(shape_dst)
        fx[f"{case}.k"], fx[f"{case}.thresh"] = k, thresh
        for key in C.KEYS:
            fx[f"{case}.{key}"] = np.asarray(r[key], dtype=np.float64 if key in C.KEYS[:2] else np.int64)
        print(f"{case:18s} rep {float(r['repeatability']):7.3f} err {float(r['localization_err']):8.5f} "
              f"N1 {r['common_src_num']:4d} N2 {r['common_dst_num']:4d} found {int(r['rep_src_num'])}/{int(r['rep_dst_num'])}")

    # what the fixture must show
    f = lambda c, key: float(fx[f"{c}.{key}"])
    assert f("both_above_k", "common_src_num") == 1000 and f("both_above_k", "common_dst_num") == 1000
    assert f("src_above_k", "common_src_num") == 1000 and f("src_above_k", "common_dst_num") < 1000
    assert f("dst_above_k", "common_src_num") < 1000 and f("dst_above_k", "common_dst_num") == 1000
    assert f("neither_above_k", "common_src_num") < 1000 and f("neither_above_k", "common_dst_num") < 1000
    assert f("k300", "common_src_num") == 300 and f("k300", "common_dst_num") == 300
    assert 0 < f("shift", "common_src_num") < 300 and 0 < f("shift", "common_dst_num") < 300
    for c in ("empty_src", "empty_dst", "both_empty", "none_within"):
        assert f(c, "repeatability") == 0.0 and f(c, "localization_err") == -1.0, c
    assert f("none_within", "common_src_num") > 0 and f("none_within", "common_dst_num") > 0
    assert f("empty_src", "common_dst_num") > 0 and f("empty_dst", "common_src_num") > 0
    assert f("both_above_k", "repeatability") > 30.0

    # adapt_homography_to_preprocessing: original sizes of several aspect ratios, both targets
    rng = np.random.default_rng(77)
    hs, shapes, warped, targets, outs = [], [], [], [], []
    for i in range(12):
        h = np.array([[1 + rng.normal() * 0.1, rng.normal() * 0.1, rng.normal() * 30],
                      [rng.normal() * 0.1, 1 + rng.normal() * 0.1, rng.normal() * 30],
                      [rng.normal() * 1e-4, rng.normal() * 1e-4, 1.0]])
        sh = np.array([rng.integers(200, 1200), rng.integers(200, 1600)])
        wsh = np.array([rng.integers(200, 1200), rng.integers(200, 1600)])
        t = [240, 320] if i % 3 else [480, 640]
        out = adapt({'homography': h, 'shape': sh, 'warped_shape': wsh}, types.SimpleNamespace(resize_shape=t))
        hs.append(h); shapes.append(sh); warped.append(wsh); targets.append(t); outs.append(out)
    fx["adapt.homography"], fx["adapt.shape"], fx["adapt.warped_shape"] = np.asarray(hs), np.asarray(shapes), np.asarray(warped)
    fx["adapt.target"], fx["adapt.out"] = np.asarray(targets), np.asarray(outs)
    assert fx["adapt.out"].dtype == np.float64

    out = os.path.join(HERE, "resize_repeat.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 400 * 1024


if __name__ == "__main__":
    main()
