#!/usr/bin/env python3
"""Record tests/golden/pair_synth.npz by running the REFERENCE's label and geometry functions.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_pair_synth_golden.py

balf/datasets/dataset_utils.py imports cv2 and imgaug (absent offline), so the function bodies are compiled from the
reference's source with ``ast`` and run unchanged, as make_golden.py does: select_k_best, labels_to_heatmap,
apply_homography_to_source_labels_torch, warp_points, filter_points, scatter_points, get_dst_point, get_window_point.  What is
NOT the reference's: the two cv2 calls of generate_homography (getRotationMatrix2D, getPerspectiveTransform) are the port's
restatements (balf_amd/datasets/dataset_utils.py), so the recorded pair geometry pins the port's draws, windows and
composition against the reference's statements, not cv2's last bits; the image warp (cv2.warpPerspective) is not recorded at
all -- the tests compare it against tests/pair_synth_common.py's integer restatement.  The lines of COCO.__getitem__ that
compose the two homographies (COCO.py:111-116, :135-142) and cut the windows (:99-125) are not a function and are restated
below word for word.

The fixture holds numbers only: the label rows of every case, per (patch, case, top_k) the two cropped heat maps, the source
patch (img / 255.0 narrowed to float32, the reference's expression) of a few cases, the 256 values of byte / 255.0, and the
geometry of seeded draws (inv_h, windows, the two float32 homographies, get_dst_point's corners, the four scalar draws and the
state of the generator after generate_homography).

STABILITY CONDITION (asserted here): torch evaluates the float32 label warp as a matrix product whose summation order and use
of fused operations are not specified.  Every warped label coordinate of every recorded case is more than 1e-3 px away from a
rounding boundary (k + 0.5) and from the filter bounds 0, W - 1 and H - 1, so that any evaluation order gives the same heat
map.  The exact cases (identity, integer translation) are excepted: for them every evaluation order is exact.  No recorded
prob has a tie at the top_k cut other than the one deliberate tie case, whose expectation is the lower-index rule, taken from
the restatement and not from the reference (NumPy's argsort is unstable there).  A candidate label seed that fails is replaced
by the next one; that is a condition on the inputs, nothing is skipped at test time.
"""
import os
import random
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from tests.golden.make_golden import ref_functions                  # noqa: E402
from tests import pair_synth_common as S                            # noqa: E402
from balf_amd.datasets import dataset_utils as DU                   # noqa: E402

REF = "/root/reference/balf/datasets/dataset_utils.py"
LABEL_FUNCS = ["select_k_best", "labels_to_heatmap", "apply_homography_to_source_labels_torch", "warp_points", "filter_points",
               "scatter_points"]
MARGIN = 1e-3
IMG_SRC_CASES = ("identity_tl", "identity_br", "rot25_half", "last_col")
GEOM_SEEDS = tuple(range(8))
GEOM_CFG = {"perspective": 0.2, "rotation": 25, "scale": 0.1}       # (the reference's config_files values are of this size)
GEOM_SHAPE, GEOM_PATCH = (240, 320, 3), 64


def stable(warped, shape):
    h, w = shape
    w64 = warped.astype(np.float64)
    frac = np.abs(w64 - np.floor(w64) - 0.5)
    edge = np.minimum.reduce([np.abs(w64[:, 0]), np.abs(w64[:, 0] - (w - 1)), np.abs(w64[:, 1]), np.abs(w64[:, 1] - (h - 1))])
    return bool(np.isfinite(w64).all() and (frac > MARGIN).all() and (edge > MARGIN).all())


def reference_geometry(seed):
    """One accepted pair of COCO.__getitem__'s loop (:53-142) on an image of GEOM_SHAPE, the generator seeded with ``seed``."""
    rng = random.Random(seed)
    ref = ref_functions(REF, ["get_dst_point", "get_window_point"], {"random": rng})
    patch_size, source_shape = GEOM_PATCH, GEOM_SHAPE
    first = None
    while True:
        state0 = rng.getstate()
        dst_point = ref["get_dst_point"](GEOM_CFG["perspective"], source_shape)
        rng.setstate(state0)
        h = DU.generate_homography(source_shape, GEOM_CFG, rng)      # (cv2's two calls: the port's restatements)
        if first is None:                                           # the first draw: what generate_homography consumes
            probe = random.Random(seed)
            ref_probe = ref_functions(REF, ["get_dst_point"], {"random": probe})
            ref_probe["get_dst_point"](GEOM_CFG["perspective"], source_shape)
            scalars = [probe.randint(-GEOM_CFG["rotation"], GEOM_CFG["rotation"]), probe.randint(-25, 50), probe.randint(-40, 40),
                       probe.randint(-40, 40)]
            assert probe.getstate() == rng.getstate()
            first = (dst_point, scalars, np.asarray(rng.getstate()[1], dtype=np.uint64))
        inv_h = np.linalg.inv(h)
        inv_h = inv_h / inv_h[2, 2]
        point_src = ref["get_window_point"](source_shape, patch_size)
        point_dst = inv_h.dot([point_src[1], point_src[0], 1.0])
        point_dst = [point_dst[1] / point_dst[2], point_dst[0] / point_dst[2]]
        if (point_dst[0] - patch_size / 2) < 0 or (point_dst[1] - patch_size / 2) < 0:
            continue
        if (point_dst[0] + patch_size / 2) > source_shape[0] or (point_dst[1] + patch_size / 2) > source_shape[1]:
            continue
        h_src_translation = np.asanyarray([[1., 0., -(int(point_src[1]) - patch_size / 2)],
                                           [0., 1., -(int(point_src[0]) - patch_size / 2)],
                                           [0., 0., 1.]])
        h_dst_translation = np.asanyarray([[1., 0., int(point_dst[1] - patch_size / 2)],
                                           [0., 1., int(point_dst[0] - patch_size / 2)],
                                           [0., 0., 1.]])
        rows_src = (int(point_src[0] - patch_size / 2), int(point_src[0] + patch_size / 2))
        cols_src = (int(point_src[1] - patch_size / 2), int(point_src[1] + patch_size / 2))
        rows_dst = (int(point_dst[0] - patch_size / 2), int(point_dst[0] + patch_size / 2))
        cols_dst = (int(point_dst[1] - patch_size / 2), int(point_dst[1] + patch_size / 2))
        if not all(b - a == patch_size for a, b in (rows_src, cols_src, rows_dst, cols_dst)):
            continue
        homography = np.dot(h_src_translation, np.dot(h, h_dst_translation))
        homography_dst_2_src = homography.astype('float32')
        homography_dst_2_src = homography_dst_2_src / homography_dst_2_src[2, 2]
        homography_src_2_dst = np.linalg.inv(homography)
        homography_src_2_dst = homography_src_2_dst.astype('float32')
        homography_src_2_dst = homography_src_2_dst / homography_src_2_dst[2, 2]
        return {"inv_h": inv_h, "win_src": np.asarray([rows_src[0], cols_src[0]]), "win_dst": np.asarray([rows_dst[0], cols_dst[0]]),
                "h_src_2_dst": homography_src_2_dst, "h_dst_2_src": homography_dst_2_src, "dst_point": first[0],
                "scalars": np.asarray(first[1]), "state": first[2]}


def main():
    ref = ref_functions(REF, LABEL_FUNCS, {"torch": torch})
    ims = S.images()
    fx = {"meta.patches": np.asarray(S.PATCHES), "meta.top_ks": np.asarray(S.TOP_KS), "meta.cases": np.asarray(list(S.cases(32))),
          "meta.geom_seeds": np.asarray(GEOM_SEEDS), "meta.geom_shape": np.asarray(GEOM_SHAPE), "meta.geom_patch": GEOM_PATCH,
          "meta.geom_cfg": np.asarray([GEOM_CFG["perspective"], GEOM_CFG["rotation"], GEOM_CFG["scale"]]),
          "norm255": np.asarray(torch.tensor(np.arange(256, dtype=np.uint8) / 255.0, dtype=torch.float32))}

    # the labels: the first candidate seed that meets the stability condition
    for ci, (name, c) in enumerate(S.cases(32).items()):
        shape = S.IMAGE_SHAPES[c["image"]]
        inv_h_t = torch.tensor(c["inv_h"], dtype=torch.float32)
        for seed in range(100 * ci, 100 * ci + 50):
            pts = S.make_labels(*c["labels"], shape, seed)
            ints = torch.tensor(pts).long()
            warped = ref["warp_points"](torch.stack((ints[:, 0], ints[:, 1]), dim=1), inv_h_t).numpy().reshape(-1, 2)
            ok = c["exact"] or stable(warped, shape)
            if ok:
                break
            print(f"{name}: label seed {seed} is within {MARGIN} px of a boundary, trying the next")
        assert ok, name
        if c["exact"]:                                              # exact means exact: integer results
            assert np.array_equal(warped, np.rint(warped)), name
        prob = pts[:, 2]
        cut = S.TOP_KS[0]
        if c["labels"][0] == "tie":
            order = np.sort(prob)[::-1]
            assert order[cut - 1] == order[cut] and (prob == order[cut]).sum() == 5, name
        elif len(prob) > cut:
            assert len(np.unique(prob)) == len(prob), name
        fx[f"labels.{name}"] = pts

    for patch in S.PATCHES:
        for name, c in S.cases(patch).items():
            im, shape = ims[c["image"]], ims[c["image"]].shape
            pts = fx[f"labels.{name}"]
            inv_h_t = torch.tensor(c["inv_h"], dtype=torch.float32)
            for top_k in S.TOP_KS:
                if c["labels"][0] == "tie" and top_k:
                    kept = pts[S.select_k_best(pts, top_k)]          # the lower-index rule: the restatement's, not the reference's
                else:
                    kept = ref["select_k_best"](pts, top_k)
                heat_src = ref["labels_to_heatmap"](kept, shape)
                heat_dst = ref["apply_homography_to_source_labels_torch"](kept, shape, inv_h_t).squeeze(0).numpy()
                assert heat_src.dtype == np.float32 and heat_dst.dtype == np.float32 and heat_dst.shape == shape[:2]
                key = f"p{patch}.{name}.k{top_k}"
                fx[f"{key}.heat_src"] = S.crop(heat_src, c["win_src"], patch).astype(np.uint8)
                fx[f"{key}.heat_dst"] = S.crop(heat_dst, c["win_dst"], patch).astype(np.uint8)
                assert set(np.unique(heat_src)) <= {0.0, 1.0} and set(np.unique(heat_dst)) <= {0.0, 1.0}
                # the restatement agrees with the reference on the full maps
                want_s, want_d = S.heatmaps(pts, top_k, shape[:2], c["inv_h"])
                assert np.array_equal(want_s, heat_src) and np.array_equal(want_d, heat_dst), key
            if name in IMG_SRC_CASES:
                src_RGB_norm = im / 255.0
                patch_t = torch.tensor(S.crop(src_RGB_norm, c["win_src"], patch), dtype=torch.float32).permute(2, 0, 1)
                fx[f"p{patch}.{name}.img_src"] = np.ascontiguousarray(patch_t.numpy())
        # what the table must show (on the restatement: the windows really exercise what their comments say)
        cs = S.cases(patch)
        e = {n: S.expected_from(patch, n, S.TOP_KS[0], fx) for n in cs}
        assert np.array_equal(e["identity_tl"][1], e["identity_tl"][0]) and np.array_equal(e["identity_br"][1], e["identity_br"][0])
        assert e["outside"][4] == 0 and not e["outside"][1].any() and not e["outside"][3].any()
        assert not e["shift_int"][1][:, :, :20].any() and not e["shift_int"][1][:, -7:, :].any() and e["shift_int"][1][:, :-7, 20:].any()
        for n in ("identity_tl", "identity_br", "mild", "mild_tie", "one_label", "dups"):
            assert e[n][2].any(), (patch, n)                       # some label lands in the source window
        assert e["mild"][3].any() and e["dups"][3].any() and e["rot25_half"][3].any()
        assert fx[f"p{patch}.identity_br.k0.heat_src"][-1, -1] == 1 and fx[f"p{patch}.identity_br.k0.heat_dst"][-1, -1] == 1
        assert fx[f"p{patch}.mild.k25.heat_src"].sum() < fx[f"p{patch}.mild.k0.heat_src"].sum()

    for seed in GEOM_SEEDS:
        for k, v in reference_geometry(seed).items():
            fx[f"geom.{seed}.{k}"] = v
        got = DU.sample_pair_geometry(GEOM_SHAPE, GEOM_CFG, GEOM_PATCH, random.Random(seed))
        for k in ("inv_h", "h_src_2_dst", "h_dst_2_src"):
            assert np.array_equal(got[k], fx[f"geom.{seed}.{k}"]), (seed, k)

    out = os.path.join(HERE, "pair_synth.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
