#!/usr/bin/env python3
"""Record tests/golden/nms_map.npz from the REFERENCE's own functions on the CPU.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    python tests/golden/make_nms_map_golden.py

The reference's benchmark_test/repeatability_tools.py cannot be imported here (torchvision is not installed), so its functions are
compiled unchanged from its source (make_golden.ref_functions):

* ``apply_nms_fast`` (:25-79) and ``get_nms_score_map_from_score_map`` (:82-100, with its ``nms_fast``) are called as they are;
  ``apply_nms_fast`` uses ``np.int``, which this NumPy no longer has: the alias is set for the call.  ASSERTED: both return the
  same map on every input -- the equivalence DESIGN.md 7aa argues, checked on the CPU.
* ``box_nms`` (:227-255) needs torchvision and ``.cuda()``: its lines that build ``boxes`` / ``scores`` (:239-241) and its
  ``keep_top_k`` / scatter lines (:246-253) are restated here around the reference's OWN pure-torch ``nms(boxes, scores, iou)``
  (:294-316, with its ``box_iou`` / ``box_area``), the implementation the reference keeps next to the torchvision call.

Inputs where the reference is defined, every candidate score distinct: nms_map_common.synthetic_scores (seeded permutations of
distinct float32 values, part of them below the threshold) at 40 x 72 and 33 x 130, and a 40 x 72 crop of a real score map of
tests/golden/natural.npz whose candidate scores are asserted pairwise distinct.  Stored: inputs, expected maps and a SHA-256 of
the inputs.  Nothing of the reference is committed: the fixture holds numbers only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_functions                                  # noqa: E402
from tests import nms_map_common as M                                               # noqa: E402

REF = "/root/reference/balf/benchmark_test/repeatability_tools.py"


def natural_crop():
    """The first 40 x 72 crop (stepping over the map) of the real score map with a few hundred candidates, all distinct."""
    key, h, w = M.NATURAL_CROP
    prob = np.load(os.path.join(HERE, "natural.npz"))[key]
    for y0 in range(0, prob.shape[0] - h + 1, h):
        for x0 in range(0, prob.shape[1] - w + 1, w):
            crop = np.ascontiguousarray(prob[y0:y0 + h, x0:x0 + w])
            cand = crop[crop >= np.float32(M.CONF)]
            if len(cand) >= 300 and len(np.unique(cand)) == len(cand):
                print(f"natural: crop of {key} at ({y0}, {x0}), {len(cand)} candidates")
                return crop
    raise AssertionError("no crop with distinct candidate scores")


def reference_box_nms(fn, prob_np, size, iou, min_prob, keep_top_k):
    prob = torch.from_numpy(prob_np)
    pts = torch.stack(torch.where(prob >= min_prob)).t()                            # :239
    boxes = torch.cat((pts - size / 2.0, pts + size / 2.0), dim=1).to(torch.float32)    # :240
    scores = prob[pts[:, 0], pts[:, 1]]                                             # :241
    indices = fn["nms"](boxes=boxes, scores=scores, iou_threshold=iou)              # :245, the reference's own nms
    pts = pts[indices, :]
    scores = scores[indices]
    if keep_top_k > 0:
        k = min(scores.shape[0], keep_top_k)
        scores, indices = torch.topk(scores, k)
        pts = pts[indices, :]
    nms_prob = torch.zeros_like(prob)
    nms_prob[pts[:, 0], pts[:, 1]] = scores
    return nms_prob.numpy()


def main():
    fn = ref_functions(REF, ["apply_nms_fast", "get_nms_score_map_from_score_map", "nms_fast", "nms", "box_iou", "box_area"],
                       {"torch": torch})
    inputs = {name: M.synthetic_scores(name) for name in M.SYNTH_SHAPES}
    inputs["natural"] = natural_crop()
    fx = {}
    for case in M.CASES:
        score = inputs[case]
        cand = score[score >= np.float32(M.CONF)]
        assert score.dtype == np.float32 and len(np.unique(cand)) == len(cand) and 0 < len(cand) < 6000, case
        fx[f"{case}.score"] = score
        for size, iou, k in M.BOX_ARGS:
            got = reference_box_nms(fn, score, size, iou, M.CONF, k)
            assert got.dtype == np.float32
            fx[f"{case}.{M.box_key(size, iou, k)}"] = got
            print(f"{case} box size {size} iou {iou} k {k}: {np.count_nonzero(got)} of {len(cand)} kept")
        for d in M.GREEDY_DISTS:
            had = hasattr(np, "int")
            if not had:
                np.int = int
            try:
                a = fn["apply_nms_fast"](score, d, M.CONF)
            finally:
                if not had:
                    del np.int
            b = fn["get_nms_score_map_from_score_map"](score, M.CONF, d)
            assert a.dtype == np.float32 and M.same_map(a, b), (case, d)                # the equivalence, on the CPU
            fx[f"{case}.greedy_d{d}"] = a
            print(f"{case} greedy dist {d}: {np.count_nonzero(a)} kept, apply_nms_fast == get_nms_score_map_from_score_map")
    fx["inputs_sha256"] = np.asarray(M.digest(*[inputs[c] for c in M.CASES]))
    np.savez_compressed(M.FIXTURE, **fx)
    print("wrote", M.FIXTURE, os.path.getsize(M.FIXTURE), "bytes")
    assert os.path.getsize(M.FIXTURE) < 1000000


if __name__ == "__main__":
    main()
