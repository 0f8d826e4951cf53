"""Batched evaluation core of the HSequences protocol: the per-pair body of ``check_val_hsequences_repeatability``
(reference balf/utils/train_utils.py:350-379) after detection, for P image pairs at once on the GPU.

Per pair, :func:`evaluate_pairs` does what that loop does with the one-pair functions of this package --
``create_common_region_masks`` -> ``check_common_points`` on both lists -> ``apply_homography_to_points`` of the kept
destination rows -> ``compute_repeatability`` -- with the same bits, but stream-ordered and without a host round trip: the
masks are evaluated at the points only (``balf_common_points_batch``) and the repeatability of all pairs runs in one sequence
of launches (``balf_repeatability_batch``).  Everything stays on the device; nothing is read back.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .._lib import BalfHipError, check, current_stream_ptr, lib, require_gpu_tensor
from .repeatability_tools import RepeatabilityBatch, _counts, compute_repeatability_batch


class CommonPoints(NamedTuple):
    src: torch.Tensor           # [P,Ns,4] float64: the kept source rows, in order; rows past the kept count are 0
    dst_to_src: torch.Tensor    # [P,Nd,4] float64: the kept destination rows warped into the source image (score carried)
    kept: torch.Tensor          # [P,2] int32: kept counts (source, destination)
    valid: torch.Tensor         # [P] int32: both kept lists are non-empty (the reference skips the pair otherwise)


class PairEvaluation(NamedTuple):
    rep_single_scale: torch.Tensor
    rep_multi_scale: torch.Tensor
    error_overlap_single_scale: torch.Tensor
    error_overlap_multi_scale: torch.Tensor
    num_points_single_scale: torch.Tensor
    num_points_multi_scale: torch.Tensor
    possible_matches: torch.Tensor
    total_num_points: torch.Tensor
    candidates_single_scale: torch.Tensor
    candidates_multi_scale: torch.Tensor
    valid: torch.Tensor
    kept: torch.Tensor


def _pair_tensor(t, dev, name, shapes_ok, dtype):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t)).to(dev)           # (a host -> device copy: pass device tensors to capture a graph)
    require_gpu_tensor(t, name)
    if t.device != dev or tuple(t.shape) not in shapes_ok:
        raise BalfHipError(f"{name} must be a {' or '.join(map(str, shapes_ok))} tensor on {dev}, got {tuple(t.shape)}")
    return t if t.dtype == dtype else t.to(dtype)


def common_points_batch(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes) -> CommonPoints:
    """``check_common_points`` of both lists against the pair's common-region masks, then ``apply_homography_to_points`` of
    the kept destination rows (``balf_common_points_batch``, include/balf_hip.h).  ``src_pts`` [P,Ns,4] / ``dst_pts``
    [P,Nd,4] float64 rows (x, y, radius, score) with counts ``src_count`` / ``dst_count`` [P] int32, ``h_dst_2_src``
    [P,3,3] float64, ``shapes`` [P,4] int32 = (h_src, w_src, h_dst, w_dst), all on the GPU."""
    for t, name in ((src_pts, "src_pts"), (dst_pts, "dst_pts")):
        require_gpu_tensor(t, name)
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] != 4:
            raise BalfHipError(f"{name} must be a [P,N,4] float64 tensor: rows (x, y, radius, score)")
    p, ns_max, nd_max = src_pts.shape[0], src_pts.shape[1], dst_pts.shape[1]
    if dst_pts.shape[0] != p or p == 0:
        raise BalfHipError(f"src_pts and dst_pts must hold the same number (> 0) of pairs, got {p} and {dst_pts.shape[0]}")
    dev = src_pts.device
    ns = _counts(src_count, p, dev, "src_count").contiguous()
    nd = _counts(dst_count, p, dev, "dst_count").contiguous()
    h = _pair_tensor(h_dst_2_src, dev, "h_dst_2_src", ((p, 3, 3), (p, 9)), torch.float64)
    sh = _pair_tensor(shapes, dev, "shapes", ((p, 4),), torch.int32)
    src_out = torch.empty_like(src_pts)
    dst_out = torch.empty_like(dst_pts)
    kept = torch.empty((p, 2), dtype=torch.int32, device=dev)
    valid = torch.empty((p,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().balf_common_points_batch(src_pts.data_ptr(), ns.data_ptr(), ns_max, dst_pts.data_ptr(), nd.data_ptr(),
                                             nd_max, p, h.data_ptr(), sh.data_ptr(), src_out.data_ptr(), dst_out.data_ptr(),
                                             kept.data_ptr(), valid.data_ptr(), current_stream_ptr(dev)),
              "balf_common_points_batch")
    return CommonPoints(src_out, dst_out, kept, valid)


def evaluate_pairs(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes, **repeat_kw) -> PairEvaluation:
    """The evaluation of P pairs after detection: :func:`common_points_batch`, then
    :func:`~balf_amd.benchmark_test.repeatability_tools.compute_repeatability_batch` on the kept source rows and the warped
    kept destination rows (``repeat_kw``: its ``overlap_err``, ``eps``, ``dist_match_thresh``, ``radious_size``,
    ``max_edges``).  Inputs as :func:`common_points_batch`: ``[P,N,4]`` rows plus counts is what
    ``multiscale.detect_batch_multiscale`` returns.  Returns the per-pair fields of ``compute_repeatability`` plus ``valid``
    and the kept counts, all device tensors: nothing is read back, and the call can be captured with ``torch.cuda.graph``.
    A pair with ``valid == 0`` is one the reference's loop skips (``continue``); it is not part of the means."""
    cp = common_points_batch(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes)
    r: RepeatabilityBatch = compute_repeatability_batch(cp.src, cp.kept[:, 0], cp.dst_to_src, cp.kept[:, 1], **repeat_kw)
    return PairEvaluation(*r, cp.valid, cp.kept)


def evaluate_val_pairs(prob_src, prob_dst, h_dst_2_src, nms_size=15, num_points=25, leg="greedy", conf_thresh=0.015,
                       **repeat_kw) -> PairEvaluation:
    """The per-pair body of ``check_val_repeatability`` (reference balf/utils/train_utils.py:232-283) after the forward, for P
    pairs at once: score maps ``prob_src`` [P,Hs,Ws] / ``prob_dst`` [P,Hd,Wd] fp32, ``h_dst_2_src`` [P,3,3] float64, on the
    GPU.  ``leg='greedy'`` is the loop's main evaluation (``get_nms_score_map_from_score_map`` with ``conf_thresh``, times
    the common-region mask, ``get_point_coordinates``), ``leg='window'`` its ``compute_repeatability_with_maximum_filter``
    (``apply_nms`` instead).  Unlike :func:`evaluate_pairs` the ``num_points`` best are chosen AFTER the mask and come out in
    raster order (``ops.val_points``); then :func:`~balf_amd.benchmark_test.repeatability_tools.compute_repeatability_batch`
    (``repeat_kw``).  Returns the same tuple as :func:`evaluate_pairs`, device tensors: ``kept`` [P,2] are the selected
    counts, ``valid`` is 1 everywhere (the reference's loop skips no pair: the selection never returns an empty list).
    Nothing synchronises or is read back; the call can be captured with ``torch.cuda.graph``."""
    from .. import ops
    dev = prob_src.device if isinstance(prob_src, torch.Tensor) else None
    if isinstance(h_dst_2_src, torch.Tensor) and h_dst_2_src.dtype != torch.float64:
        h_dst_2_src = h_dst_2_src.to(torch.float64)
    elif not isinstance(h_dst_2_src, torch.Tensor):
        h_dst_2_src = torch.as_tensor(np.asarray(h_dst_2_src, dtype=np.float64)).to(dev)   # (host -> device: not capturable)
    src, dst, count = ops.val_points(prob_src, prob_dst, h_dst_2_src.contiguous(), nms_size, num_points, leg, conf_thresh)
    r: RepeatabilityBatch = compute_repeatability_batch(src, count[:, 0], dst, count[:, 1], **repeat_kw)
    return PairEvaluation(*r, torch.ones_like(count[:, 0]), count)
