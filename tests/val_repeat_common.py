"""Shared by tests/test_val_repeat_host.py, tests/test_val_repeat_gpu.py and tests/golden/make_val_golden.py: the fixture
val_repeat.npz, the loader built from it, and the per-pair body of check_val_repeatability stated twice -- from the CPU
oracle's pieces, and from this package's one-pair GPU functions (the loop that evaluate_val_pairs replaces)."""
import os

import numpy as np
import torch

from balf_amd.utils import synth
from oracle import oracle as O

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "val_repeat.npz")
LEGS = ("greedy", "window")
REP_KEYS = ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale",
            "possible_matches")
COUNT_KEYS = ("num_points_single_scale", "num_points_multi_scale", "total_num_points")
CONF_THRESH = 0.015
# h_dst_2_src of elements 1.. of a loader batch (the reference never looks at them)
EXTRA_H = np.array([[0.9, 0.1, 3.0], [-0.1, 1.1, -2.0], [1e-4, 2e-5, 1.0]])


def val_case_extra(h, w, batch, element):
    """uint8 gray image of element ``element`` >= 1 of loader batch ``batch`` (regenerated from the seed on both sides)."""
    return synth.synthetic_gray_u8(h, w, 900 + 10 * batch + element)


def to_input(gray_u8):
    """uint8 gray [H,W] -> the loader's [3,H,W] float32 image: gray / 255 replicated to three channels."""
    g = torch.from_numpy(gray_u8.astype(np.float32) / np.float32(255.0))
    return g[None].expand(3, -1, -1).contiguous()


def loader_batches(image_src, image_dst, h_dst_2_src, batch_sizes):
    """The 6-tuples the reference's loop unpacks, one per pair: element 0 is the pair, elements 1.. are other images."""
    batches = []
    for bi, (s, d, h, bsz) in enumerate(zip(image_src, image_dst, h_dst_2_src, batch_sizes)):
        srcs, dsts, hs = [to_input(s)], [to_input(d)], [np.asarray(h, np.float64)]
        for e in range(1, int(bsz)):
            srcs.append(to_input(val_case_extra(*s.shape, bi, e)))
            dsts.append(to_input(val_case_extra(*d.shape, bi, e + 5)))
            hs.append(EXTRA_H)
        hh = torch.from_numpy(np.stack(hs))
        batches.append((torch.stack(srcs), torch.stack(dsts), torch.zeros((int(bsz), 1) + s.shape),
                        torch.zeros((int(bsz), 1) + d.shape), torch.linalg.inv(hh), hh))
    return batches


def fixture():
    return np.load(FIXTURE)


def fixture_loader(g):
    names = [str(n) for n in g["meta.names"]]
    return loader_batches([g[f"{n}.image_src"] for n in names], [g[f"{n}.image_dst"] for n in names],
                          [g[f"{n}.h_dst_2_src"] for n in names], g["meta.batch_sizes"])


def map_names(g):
    """Every case with recorded score maps: the loader's pairs and the score-map-only ones."""
    return [str(n) for n in g["meta.names"]] + [str(n) for n in g["meta.map_only_names"]]


# ---- the per-pair body from the CPU oracle's pieces -------------------------------------------------------------------------
def oracle_nms_map(prob, nms_size, leg):
    if leg == "window":
        return O.apply_nms(prob, nms_size)
    idx, sc = O.greedy_nms(prob, CONF_THRESH, nms_size)                 # get_nms_score_map_from_score_map: kept points scattered
    out = np.zeros_like(prob)
    out.ravel()[idx] = sc
    return out


def oracle_pair(prob_src, prob_dst, h, nms_size, num_points, leg):
    """-> (src rows, dst rows, dst rows warped, compute_repeatability dict), train_utils.py:232-257 / :171-189."""
    ms, md = O.create_common_region_masks(h, prob_src.shape, prob_dst.shape, numpy_inverse=False)
    rows = []
    for prob, mask in ((prob_src, ms), (prob_dst, md)):
        masked = np.multiply(oracle_nms_map(prob, nms_size, leg), mask)
        idx, sc = O.select_topk(masked, num_points)
        rows.append(O.points_xysr(idx, sc, prob.shape[1]))
    warped = O.apply_homography_to_points(rows[1], h)
    return rows[0], rows[1], warped, O.compute_repeatability(rows[0], warped)


# ---- the same body from this package's one-pair GPU functions (what a caller had to write before evaluate_val_pairs) ------
def gpu_loop_pair(prob_src, prob_dst, h, nms_size, num_points, leg):
    """``prob_*``: [H,W] float32 NumPy score maps.  -> (src rows, dst rows warped, compute_repeatability dict)."""
    from balf_amd import ops
    from balf_amd.benchmark_test import geometry_tools, repeatability_tools
    from balf_amd.utils import test_utils
    ms, md = geometry_tools.create_common_region_masks(h, prob_src.shape, prob_dst.shape)
    rows = []
    for prob, mask in ((prob_src, ms), (prob_dst, md)):
        if leg == "window":
            nms = test_utils.apply_nms(prob, nms_size)
        else:
            hh, ww = prob.shape
            t = torch.from_numpy(np.ascontiguousarray(prob)).cuda().unsqueeze(0)
            idx, score, _, count, total = ops.greedy_nms(t, 0, 0, hh, ww, 0, CONF_THRESH, nms_size, min(16384, hh * ww), 0)
            n = int(count[0])
            assert int(total[0]) == n
            nms = np.zeros_like(prob)
            nms.ravel()[idx[0, :n].cpu().numpy().astype(np.int64)] = score[0, :n].cpu().numpy()
        rows.append(test_utils.get_point_coordinates(np.multiply(nms, mask), num_points=num_points, order_coord='xysr'))
    warped = geometry_tools.apply_homography_to_points(rows[1], h)
    return rows[0], warped, repeatability_tools.compute_repeatability(rows[0], warped)
