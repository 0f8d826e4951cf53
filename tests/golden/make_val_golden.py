#!/usr/bin/env python3
"""Record tests/golden/val_repeat.npz by running the REFERENCE's check_val_repeatability and the functions under it.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_val_golden.py

balf/utils/train_utils.py, benchmark_test/repeatability_tools.py and benchmark_test/geometry_tools.py import tqdm /
torchvision / cv2 / torchgeometry (absent offline), so their function bodies are compiled from the reference's source with
``ast`` and run unchanged, as make_golden.py does: get_nms_score_map_from_score_map, nms_fast, apply_nms,
get_point_coordinates, find_index_higher_scores, apply_homography_to_points, getAff, compute_repeatability,
compute_repeatability_with_maximum_filter and check_val_repeatability.  The one piece that is not the reference's is
create_common_region_masks: cv2 is absent, the masks come from oracle.create_common_region_masks(numpy_inverse=False)
(that leg stays "parity unpinned").  tqdm is replaced by a pass-through object.

The fixture holds numbers only.  Per pair (= element 0 of one loader batch): the input images (uint8 gray; the loader feeds
gray / 255 replicated to three channels as float32), h_dst_2_src, the two score maps of the reference model with the
synthetic weights (seed 3), the selected rows of both legs before and after the homography, the repeatability results; and
the ten return values of check_val_repeatability over the whole loader.  One more case, "zero", holds all-zero score maps
only (the selection's raster fallback, which no image reaches with these weights: see main).  Elements 1.. of a loader batch are regenerated from
seeds (tests/val_repeat_common.py: val_case_extra) -- the reference never looks at them.

STABILITY CONDITION (asserted here): the GPU forward is within 6e-6 of the reference's score map, which could flip a near-tie
of the selection.  Every recorded pair's selected point sets (both legs, both sides) are unchanged when the reference's score
maps are perturbed by uniform noise of +-2e-5 (the split-f16 gate), in STABILITY_SEEDS seeds.  A candidate image seed that
fails is replaced by the next one; that is a condition on the inputs, nothing is skipped at test time.
"""
import os
import sys
import time
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from tests.golden.make_golden import ref_functions, ref_model       # noqa: E402  (puts the reference on sys.path)
from balf_amd.utils import synth                                    # noqa: E402
from oracle import oracle as O                                      # noqa: E402
from tests.val_repeat_common import loader_batches, to_input       # noqa: E402

NMS_SIZE, NUM_POINTS, WEIGHT_SEED = 15, 25, 3
STABILITY_SEEDS, NOISE = 4, 2e-5
REF = "/root/reference/balf/"


class _Tqdm:
    """tqdm(iterable, total=, desc=) as the loop uses it: iteration, update, set_description, set_postfix."""

    def __init__(self, it, total=None, desc=None):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def update(self, *a, **k):
        pass

    set_description = set_postfix = update


def reference_namespace():
    from scipy.ndimage import maximum_filter
    rt = ref_functions(REF + "benchmark_test/repeatability_tools.py",
                       ["get_nms_score_map_from_score_map", "nms_fast", "apply_nms", "compute_repeatability",
                        "intersection_area", "union_area"], {"maximum_filter": maximum_filter})
    gt = ref_functions(REF + "benchmark_test/geometry_tools.py",
                       ["get_point_coordinates", "find_index_higher_scores", "apply_homography_to_points", "getAff"])
    gt["create_common_region_masks"] = lambda h, ss, sd: O.create_common_region_masks(h, ss, sd, numpy_inverse=False)
    ns = {"torch": torch, "time": time, "tqdm": _Tqdm, "torchvision": None,
          "repeatability_tools": types.SimpleNamespace(**rt), "geometry_tools": types.SimpleNamespace(**gt)}
    tu = ref_functions(REF + "utils/train_utils.py", ["check_val_repeatability", "compute_repeatability_with_maximum_filter"], ns)
    return rt, gt, tu


def homography(kind, hd, wd):
    """h_dst_2_src (destination pixel -> source pixel)."""
    if kind == "mild":
        return np.array([[1.02, 0.03, -2.5], [-0.02, 0.99, 3.0], [4e-5, -3e-5, 1.0]])
    if kind == "mild2":
        return np.array([[0.97, -0.04, 6.0], [0.05, 1.01, -4.0], [-5e-5, 6e-5, 1.0]])
    if kind == "thin":                       # a large shift: the common region is a thin strip
        return np.array([[1.0, 0.02, wd - 42.0], [0.01, 1.0, 2.0], [0.0, 0.0, 1.0]])
    if kind == "rotate":                     # 35 degrees about the centre with a zoom: a clearly different last pair
        c, s = np.cos(np.deg2rad(35.0)) * 1.25, np.sin(np.deg2rad(35.0)) * 1.25
        cx, cy = (wd - 1) / 2.0, (hd - 1) / 2.0
        return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0.0, 0.0, 1.0]])
    raise ValueError(kind)


def warp_u8(src_u8, h_dst_2_src, hd, wd):
    """The destination image: the source resampled (bilinear, 0 outside) at h_dst_2_src (x, y, 1)."""
    ys, xs = np.mgrid[0:hd, 0:wd].astype(np.float64)
    den = h_dst_2_src[2, 0] * xs + h_dst_2_src[2, 1] * ys + h_dst_2_src[2, 2]
    sx = (h_dst_2_src[0, 0] * xs + h_dst_2_src[0, 1] * ys + h_dst_2_src[0, 2]) / den
    sy = (h_dst_2_src[1, 0] * xs + h_dst_2_src[1, 1] * ys + h_dst_2_src[1, 2]) / den
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = sx - x0, sy - y0
    s = src_u8.astype(np.float64)
    sh, sw = s.shape

    def at(yy, xx):
        ok = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        return np.where(ok, s[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0.0)

    v = at(y0, x0) * (1 - ax) * (1 - ay) + at(y0, x0 + 1) * ax * (1 - ay) + at(y0 + 1, x0) * (1 - ax) * ay + at(y0 + 1, x0 + 1) * ax * ay
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# (name, kind of homography or None for black, source shape, destination shape, loader batch size)
PAIRS = (("mild", "mild", (128, 128), (128, 128), 2),
         ("thin", "thin", (128, 128), (128, 128), 1),
         ("black", None, (128, 128), (128, 128), 3),
         ("shapes", "mild2", (128, 128), (128, 192), 1),
         ("mild_b", "mild2", (128, 128), (128, 128), 2),
         ("last", "rotate", (128, 128), (128, 128), 1))


def select_rows(rt, gt, prob, mask, leg):
    """One side of one leg exactly as the loop states it (train_utils.py:242-251 / :178-185)."""
    if leg == "greedy":
        nms = rt["get_nms_score_map_from_score_map"](prob, conf_thresh=0.015, nms_size=NMS_SIZE)
    else:
        nms = rt["apply_nms"](prob, NMS_SIZE)
    return gt["get_point_coordinates"](np.multiply(nms, mask), num_points=NUM_POINTS, order_coord='xysr')


def pair_record(rt, gt, prob_s, prob_d, h):
    ms, md = gt["create_common_region_masks"](h, prob_s.shape + (3,), prob_d.shape + (3,))
    out = {}
    for leg in ("greedy", "window"):
        src = select_rows(rt, gt, prob_s, ms, leg)
        dst = select_rows(rt, gt, prob_d, md, leg)
        warped = gt["apply_homography_to_points"](dst, h)
        r = rt["compute_repeatability"](src, warped)
        out[leg] = (src, dst, warped, r)
    return out


def point_sets(rec):
    return [tuple(map(tuple, np.asarray(rec[leg][k])[:, :2])) for leg in ("greedy", "window") for k in (0, 1)]


def main():
    rt, gt, tu = reference_namespace()
    model, _ = ref_model(WEIGHT_SEED)
    fx = {"meta.nms_size": NMS_SIZE, "meta.num_points": NUM_POINTS, "meta.weight_seed": WEIGHT_SEED,
          "meta.names": np.asarray([p[0] for p in PAIRS]), "meta.batch_sizes": np.asarray([p[4] for p in PAIRS])}
    for bi, (name, kind, (hs, ws), (hd, wd), bsz) in enumerate(PAIRS):
        for seed in range(40 + 20 * bi, 60 + 20 * bi):            # candidate inputs; the first stable one is recorded
            if kind is None:
                h = homography("mild", hd, wd)
                src_u8, dst_u8 = np.zeros((hs, ws), np.uint8), np.zeros((hd, wd), np.uint8)
            else:
                h = homography(kind, hd, wd)
                src_u8 = synth.synthetic_gray_u8(hs, ws, seed, blur=7)
                dst_u8 = warp_u8(src_u8, h, hd, wd)
            with torch.no_grad():
                prob_s = model(to_input(src_u8)[None])["prob"][0].numpy()
                prob_d = model(to_input(dst_u8)[None])["prob"][0].numpy()
            rec = pair_record(rt, gt, prob_s, prob_d, h)
            want = point_sets(rec)
            stable = True
            for s in range(STABILITY_SEEDS):
                rng = np.random.default_rng([77, bi, s])
                ps = (prob_s + rng.uniform(-NOISE, NOISE, prob_s.shape)).astype(np.float32)
                pd = (prob_d + rng.uniform(-NOISE, NOISE, prob_d.shape)).astype(np.float32)
                stable = stable and point_sets(pair_record(rt, gt, ps, pd, h)) == want
            if stable:
                break
            print(f"{name}: image seed {seed} is not stable under +-{NOISE} noise, trying the next")
        assert stable, name
        fx[f"{name}.image_src"], fx[f"{name}.image_dst"], fx[f"{name}.h_dst_2_src"] = src_u8, dst_u8, h
        fx[f"{name}.prob_src"], fx[f"{name}.prob_dst"] = prob_s, prob_d
        for leg, (src, dst, warped, r) in rec.items():
            fx[f"{name}.{leg}.src"], fx[f"{name}.{leg}.dst"], fx[f"{name}.{leg}.dst_to_src"] = src, dst, warped
            for k in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale",
                      "possible_matches", "num_points_single_scale", "num_points_multi_scale", "total_num_points"):
                fx[f"{name}.{leg}.{k}"] = np.asarray(r[k])
            print(f"{name:7s} {leg:6s} rows {len(src):3d}/{len(dst):3d} rep_s {float(r['rep_single_scale']):6.2f} "
                  f"rep_m {float(r['rep_multi_scale']):6.2f} possible {r['possible_matches']}")

    # The raster fallback (no positive value in the masked map).  With the synthetic weights even a black image has a structured
    # score map (the token mixing is position dependent), so the all-black pair above does NOT reach it: it is recorded from
    # the reference's functions on all-zero score maps, a score-map-only case (no images; not part of the loader run).
    zero = np.zeros((128, 128), np.float32)
    fx["zero.prob_src"], fx["zero.prob_dst"], fx["zero.h_dst_2_src"] = zero, zero, homography("mild", 128, 128)
    for leg, (src, dst, warped, r) in pair_record(rt, gt, zero, zero, fx["zero.h_dst_2_src"]).items():
        fx[f"zero.{leg}.src"], fx[f"zero.{leg}.dst"], fx[f"zero.{leg}.dst_to_src"] = src, dst, warped
        for k in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale",
                  "possible_matches", "num_points_single_scale", "num_points_multi_scale", "total_num_points"):
            fx[f"zero.{leg}.{k}"] = np.asarray(r[k])
    fx["meta.map_only_names"] = np.asarray(["zero"])

    names = [p[0] for p in PAIRS]
    batches = loader_batches([fx[f"{n}.image_src"] for n in names], [fx[f"{n}.image_dst"] for n in names],
                             [fx[f"{n}.h_dst_2_src"] for n in names], fx["meta.batch_sizes"])
    assert max(len(b[0]) for b in batches) > 1
    ten = tu["check_val_repeatability"](batches, model, "cpu", None, 0, nms_size=NMS_SIZE, num_points=NUM_POINTS)
    fx["loader.ten"] = np.asarray([float(v) for v in ten])
    print("ten:", fx["loader.ten"])

    # what the fixture must show
    g_mean = [np.mean([float(fx[f"{n}.greedy.{k}"]) for n in names])
              for k in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale", "possible_matches")]
    assert np.allclose(fx["loader.ten"][:5], g_mean, rtol=0, atol=1e-12)                      # means over element 0 of every batch
    w_last = [float(fx[f"last.window.{k}"]) for k in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale",
                                                      "error_overlap_multi_scale", "possible_matches")]
    assert np.array_equal(fx["loader.ten"][5:], w_last)                                        # the _nms five: the last pair only
    w_mean = [np.mean([float(fx[f"{n}.window.{k}"]) for n in names]) for k in ("rep_single_scale", "possible_matches")]
    assert abs(w_last[0] - w_mean[0]) > 1.0 or abs(w_last[4] - w_mean[1]) > 1.0, (w_last, w_mean)
    assert float(fx["mild.greedy.rep_single_scale"]) > 50.0
    for leg in ("greedy", "window"):
        assert 0 < len(fx[f"thin.{leg}.src"]) < NUM_POINTS and 0 < len(fx[f"thin.{leg}.dst"]) < NUM_POINTS, leg   # fewer than K positive
        assert len(fx[f"zero.{leg}.src"]) == NUM_POINTS and not fx[f"zero.{leg}.src"][:, 3].any()               # the raster fallback
        assert np.array_equal(fx[f"zero.{leg}.src"][:, 0], np.arange(NUM_POINTS))
        assert len(fx[f"mild.{leg}.src"]) == NUM_POINTS
    out = os.path.join(HERE, "val_repeat.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
