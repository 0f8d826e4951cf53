"""Batched evaluation core of the HSequences protocol: the per-pair body of ``check_val_hsequences_repeatability``
(reference balf/utils/train_utils.py:350-379) after detection, for P image pairs at once on the GPU.

Per pair, :func:`evaluate_pairs` does what that loop does with the one-pair functions of this package --
``create_common_region_masks`` -> ``check_common_points`` on both lists -> ``apply_homography_to_points`` of the kept
destination rows -> ``compute_repeatability`` -- with the same bits, but stream-ordered and without a host round trip: the
masks are evaluated at the points only (``balf_common_points_batch``) and the repeatability of all pairs runs in one sequence
of launches (``balf_repeatability_batch``).  Everything stays on the device; nothing is read back.

:func:`evaluate_matching_pairs` adds the matching score of the same pairs (the ``mma`` / ``mma_corr`` /
``num_matches`` / ``num_mutual_corresp`` / ``avg_mma`` fields of the reference's result record, which its public tree never
fills): the filter also reports which original row each kept row was (``balf_common_points_index_batch``), the per-image
descriptors are gathered through that, matched (``ops.match_smnn_batch``) and the matches verified against the homography
(``balf_match_accuracy_batch``).  :func:`evaluate_matching_hsequences` is the driver over a dataset.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from .._lib import BalfHipError, launch, require_gpu_tensor
from . import _chunked
from ._chunked import detection_rows  # noqa: F401
from .metrics_results import create_metrics_results
from .repeatability_tools import RepeatabilityBatch, _counts, compute_repeatability_batch
from .test_utils import RESIZE_RESULT_KEYS, create_resize_metrics_results


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


class CommonPointsIndex(NamedTuple):
    src: torch.Tensor           # the four fields of CommonPoints, bit-identical to common_points_batch's
    dst_to_src: torch.Tensor
    kept: torch.Tensor
    valid: torch.Tensor
    src_index: torch.Tensor     # [P,Ns] int32: the row of src_pts each kept source row came from, -1 past the kept count
    dst_index: torch.Tensor     # [P,Nd] int32: likewise for the destination rows


def _common_points_args(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes):
    """The checked inputs and the four outputs both filter calls share -> (the outputs as a CommonPoints, the leading
    arguments of launch() up to valid_dev)."""
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
    out = CommonPoints(torch.empty_like(src_pts), torch.empty_like(dst_pts),
                       torch.empty((p, 2), dtype=torch.int32, device=dev), torch.empty((p,), dtype=torch.int32, device=dev))
    return out, (src_pts, ns, ns_max, dst_pts, nd, nd_max, p, h, sh, *out)


def common_points_batch(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes) -> CommonPoints:
    """``check_common_points`` of both lists against the pair's common-region masks, then ``apply_homography_to_points`` of
    the kept destination rows (``balf_common_points_batch``, include/balf_hip.h).  ``src_pts`` [P,Ns,4] / ``dst_pts``
    [P,Nd,4] float64 rows (x, y, radius, score) with counts ``src_count`` / ``dst_count`` [P] int32, ``h_dst_2_src``
    [P,3,3] float64, ``shapes`` [P,4] int32 = (h_src, w_src, h_dst, w_dst), all on the GPU."""
    out, args = _common_points_args(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes)
    launch("balf_common_points_batch", src_pts.device, *args)
    return out


def common_points_index_batch(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes) -> CommonPointsIndex:
    """:func:`common_points_batch` -- same inputs, the same four outputs bit for bit -- plus ``src_index`` [P,Ns] /
    ``dst_index`` [P,Nd] int32: the original row of each kept row in kept order, -1 past the kept count
    (``balf_common_points_index_batch``).  Whatever was computed per detected row -- a descriptor -- follows its row into
    the kept list through them."""
    out, args = _common_points_args(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes)
    dev = src_pts.device
    src_index = torch.empty(src_pts.shape[:2], dtype=torch.int32, device=dev)
    dst_index = torch.empty(dst_pts.shape[:2], dtype=torch.int32, device=dev)
    launch("balf_common_points_index_batch", dev, *args, src_index, dst_index)
    return CommonPointsIndex(*out, src_index, dst_index)


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


# ---- the matching score ------------------------------------------------------------------------------------------
MAX_THRESHOLDS = 16


class MatchingEvaluation(NamedTuple):
    """Per-pair results of :func:`evaluate_matching_pairs`, device tensors: every field of :class:`PairEvaluation`, then the
    matching score."""
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
    num_mutual_corresp: torch.Tensor    # [P] int32: M, the mutual ratio-test matches between the kept lists
    num_matches: torch.Tensor           # [P] int32: those within pixel_threshold
    correct: torch.Tensor               # [P,T] int32: those within each threshold
    mma: torch.Tensor                   # [P] float64: num_matches / M (0 for M == 0)
    mma_corr: torch.Tensor              # [P] float64: num_matches / possible_matches (0 for possible_matches == 0)
    avg_mma: torch.Tensor               # [P] float64: mean over the thresholds of correct / M (0 for M == 0)
    match_idx: torch.Tensor             # [P,cap,2] int32: (row of the kept source list, row of the kept destination list), -1 padded
    match_err: torch.Tensor             # [P,cap] float64: reprojection error in source pixels, NaN past M


def _thresholds(thresholds):
    """-> (the thresholds as Python floats, as a ctypes array): 1..16 of them, >= 0 and strictly ascending."""
    ths = [float(t) for t in thresholds]
    if not 1 <= len(ths) <= MAX_THRESHOLDS:
        raise BalfHipError(f"between 1 and {MAX_THRESHOLDS} thresholds, got {len(ths)}")
    if not ths[0] >= 0.0 or any(not b > a for a, b in zip(ths, ths[1:])):
        raise BalfHipError(f"thresholds must be >= 0 and strictly ascending, got {ths}")
    return ths, (C.c_double * len(ths))(*ths)


def _threshold_index(thresholds, pixel_threshold):
    """-> (the thresholds as Python floats, the position of ``pixel_threshold`` among them)."""
    ths, _ = _thresholds(thresholds)
    if float(pixel_threshold) not in ths:
        raise BalfHipError(f"pixel_threshold {pixel_threshold} is not one of the thresholds {ths}")
    return ths, ths.index(float(pixel_threshold))


def match_accuracy_batch(src, dst, kept, match_idx, match_count, thresholds):
    """The matches of P pairs verified against the homography (``balf_match_accuracy_batch``, include/balf_hip.h).  ``src``
    [P,Ns,4] / ``dst`` [P,Nd,4] float64: the kept source rows and the kept destination rows warped into the source image
    (:func:`common_points_index_batch`), ``kept`` [P,2] int32 their lengths; ``match_idx`` [P,cap,2] int32 / ``match_count``
    [P] int32 as ``ops.match_smnn_batch`` returns them; ``thresholds``: 1..16 ascending pixel thresholds on the host.
    Returns (``err`` [P,cap] float64: ``sqrt(dx*dx + dy*dy)`` per match, NaN past the count and for an index outside the kept
    lists; ``correct`` [P,T] int32: the matches with ``err <= thresholds[k]``).  Nothing is read back."""
    ths, th_arr = _thresholds(thresholds)
    for t, name in ((src, "src"), (dst, "dst")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] != 4:
            raise BalfHipError(f"{name} must be a [P,N,4] float64 tensor: rows (x, y, radius, score)")
    p = src.shape[0]
    if dst.shape[0] != p or p == 0:
        raise BalfHipError(f"src and dst must hold the same number (> 0) of pairs, got {p} and {dst.shape[0]}")
    if not isinstance(match_idx, torch.Tensor) or match_idx.dtype != torch.int32 or match_idx.dim() != 3 or \
            match_idx.shape[0] != p or match_idx.shape[2] != 2:
        raise BalfHipError(f"match_idx must be a [{p},cap,2] int32 tensor")
    if not isinstance(kept, torch.Tensor) or kept.dtype != torch.int32 or tuple(kept.shape) != (p, 2):
        raise BalfHipError(f"kept must be a [{p},2] int32 tensor")
    dev = src.device
    for t, name in ((src, "src"), (dst, "dst"), (kept, "kept"), (match_idx, "match_idx")):
        require_gpu_tensor(t, name)
        if t.device != dev:
            raise BalfHipError(f"{name} must be on {dev} like src, got {t.device}")
    count = _counts(match_count, p, dev, "match_count").contiguous()
    cap = match_idx.shape[1]
    err = torch.empty((p, cap), dtype=torch.float64, device=dev)
    correct = torch.empty((p, len(ths)), dtype=torch.int32, device=dev)
    if cap == 0:
        return err, correct.zero_()
    launch("balf_match_accuracy_batch", dev, src, src.shape[1], dst, dst.shape[1], kept, match_idx, count, cap, p, th_arr, len(ths),
           err, correct)
    return err, correct


def _ratio(num, den):
    """num / den in float64 per pair, 0 where den == 0 (int32 in: the quotient of the exact integers, rounded once)."""
    den = den.to(torch.float64)
    zero = den == 0
    return torch.where(zero, torch.zeros_like(den), num.to(torch.float64) / torch.where(zero, torch.ones_like(den), den))


def evaluate_matching_pairs(src_pts, src_count, src_desc, dst_pts, dst_count, dst_desc, h_dst_2_src, shapes, th=0.99,
                            thresholds=range(1, 11), pixel_threshold=5, **repeat_kw) -> MatchingEvaluation:
    """:func:`evaluate_pairs` plus the matching score of the same P pairs.  Inputs as :func:`evaluate_pairs`,
    and ``src_desc`` [P,Ns,128] / ``dst_desc`` [P,Nd,128] float32: the descriptor of every DETECTED row, computed once per
    image (``desc[pair_src_image]`` is what the driver passes).  Per pair:

    * the common-region filter reports the original row of each kept row (:func:`common_points_index_batch`) and each kept
      row takes that row's descriptor (a gather on the device);
    * ``ops.match_smnn_batch`` of the kept source descriptors against the kept destination descriptors with ratio ``th``
      (0.99 is the demo's value; ``th >= 1`` keeps every mutual nearest-neighbour pair) gives M matches (i, j);
    * ``match_err`` = the distance in source pixels between kept source row i and warped kept destination row j, ``correct[k]``
      = the matches within ``thresholds[k]`` (:func:`match_accuracy_batch`; ascending, at most 16, ``pixel_threshold`` one of
      them);
    * ``num_mutual_corresp`` = M, ``num_matches`` = correct at ``pixel_threshold``, ``mma`` = num_matches / M, ``mma_corr`` =
      num_matches / possible_matches, ``avg_mma`` = the ratios correct[k] / M summed in ascending k, divided by T; a ratio with
      a zero denominator is 0.

    A pair with ``valid == 0`` has M = 0; it is left out of every mean, as in the repeatability loop.  Returns device tensors,
    reads nothing back, and can be captured with ``torch.cuda.graph`` when every input is a device tensor."""
    from .. import ops
    ths, k_star = _threshold_index(thresholds, pixel_threshold)
    for d, pts, name in ((src_desc, src_pts, "src_desc"), (dst_desc, dst_pts, "dst_desc")):
        if not isinstance(d, torch.Tensor) or not isinstance(pts, torch.Tensor) or d.dim() != 3 or d.shape[2] != 128 or \
                tuple(d.shape[:2]) != tuple(pts.shape[:2]):
            raise BalfHipError(f"{name} must be a [P,N,128] tensor: one descriptor per row of the point list")
        require_gpu_tensor(d, name)
    cp = common_points_index_batch(src_pts, src_count, dst_pts, dst_count, h_dst_2_src, shapes)
    r: RepeatabilityBatch = compute_repeatability_batch(cp.src, cp.kept[:, 0], cp.dst_to_src, cp.kept[:, 1], **repeat_kw)

    def kept_rows(desc, index):                                  # (rows past the kept count: row 0's descriptor, never matched)
        return torch.gather(desc.float(), 1, index.clamp(min=0).to(torch.int64).unsqueeze(2).expand(-1, -1, 128))

    _, match_idx, m = ops.match_smnn_batch(kept_rows(src_desc, cp.src_index), cp.kept[:, 0],
                                           kept_rows(dst_desc, cp.dst_index), cp.kept[:, 1], float(th))
    err, correct = match_accuracy_batch(cp.src, cp.dst_to_src, cp.kept, match_idx, m, ths)
    num_matches = correct[:, k_star]
    avg = _ratio(correct[:, 0], m)
    for k in range(1, len(ths)):                                 # (in this order: the summation is part of the definition)
        avg = avg + _ratio(correct[:, k], m)
    return MatchingEvaluation(*r, cp.valid, cp.kept, m, num_matches, correct, _ratio(num_matches, m),
                              _ratio(num_matches, r.possible_matches), avg / float(len(ths)), match_idx, err)


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


# ---- the resize protocol (reference configs/config_hpatches.py: parse_resize_eval_config) -----------------------------------
def evaluate_resize_pairs(src_pts, src_count, dst_pts, dst_count, h, shapes, keep_k_points=1000, distance_thresh=5,
                          h_inv=None, order="xyrs"):
    """The resize-protocol metric of P pairs after detection, device in, device out:
    :func:`~balf_amd.benchmark_test.repeatability_tools.compute_resize_repeatability_batch` on ``[P,N,4]`` float64 rows
    (x, y, radius, score) plus counts, the layout of this package's detectors (``order='rcp'`` for the reference's
    (row, col, prob) rows).  ``h`` [P,3,3] maps source to destination pixels; pass ``h_inv`` too (both device tensors) to keep
    the call free of host work and capturable with ``torch.cuda.graph``.  Returns a ``ResizeRepeatabilityBatch`` of device
    tensors; nothing is read back."""
    from .repeatability_tools import compute_resize_repeatability_batch
    return compute_resize_repeatability_batch(src_pts, src_count, dst_pts, dst_count, h, shapes, keep_k_points,
                                              distance_thresh, h_inv=h_inv, order=order)


def _as_rgb_u8(img):
    """A loader image (``*_BGR``: gray [H,W] / [H,W,1] or BGR [H,W,3] uint8) as the detector's input: gray as it is, colour
    with the channels reversed to RGB (the reference converts BGR to RGB before detection)."""
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    return np.ascontiguousarray(a[:, :, ::-1]) if a.ndim == 3 else np.ascontiguousarray(a)


def _resize_chunk(seqs, model, device, resize_shape, top_k, pixel_threshold, nms_size, border_size, batch_size):
    """One chunk of sequences -> the RESIZE_RESULT_KEYS per pair on the host (one read), in (sequence, destination) order."""
    from types import SimpleNamespace
    from ..datasets import dataset_utils
    from ..pipeline import detect_batch_u8
    th, tw = int(resize_shape[0]), int(resize_shape[1])
    args = SimpleNamespace(resize_shape=[th, tw])
    images, pair_src, pair_dst, hs = [], [], [], []
    for s in seqs:
        src = _as_rgb_u8(s['im_src_BGR'])
        i_src = len(images)
        images.append(src)
        for dst, h in zip(s['images_dst_BGR'], s['homographies']):
            dst = _as_rgb_u8(dst)
            pair_src.append(i_src)
            pair_dst.append(len(images))
            images.append(dst)
            hs.append(dataset_utils.adapt_homography_to_preprocessing(
                {'homography': np.asarray(h), 'shape': np.array(src.shape[:2]), 'warped_shape': np.array(dst.shape[:2])}, args))
    if not hs:
        return _chunked.Table(RESIZE_RESULT_KEYS)
    if len({im.ndim for im in images}) != 1:                     # gray and colour in one chunk: gray replicated to 3 channels
        images = [im if im.ndim == 3 else np.repeat(im[:, :, None], 3, axis=2) for im in images]
    batch = dataset_utils.ratio_preserving_resize_batch(images, (th, tw), device)
    rows, counts = [], []
    for b0 in range(0, batch.shape[0], batch_size):
        idx, score, count, _ = detect_batch_u8(model, batch[b0:b0 + batch_size], border_size, nms_size, top_k)
        rows.append(detection_rows(idx, score, count, tw))
        counts.append(count)
    rows, counts = torch.cat(rows), torch.cat(counts)
    i_s, i_d = _chunked.pair_index(pair_src, pair_dst, rows.device)
    shapes = np.tile(np.asarray([th, tw, th, tw], dtype=np.int32), (len(hs), 1))
    r = evaluate_resize_pairs(rows[i_s], counts[i_s], rows[i_d], counts[i_d], np.stack(hs), shapes, top_k, pixel_threshold)
    return _chunked.host_table(r, RESIZE_RESULT_KEYS)


@torch.no_grad()
def evaluate_resize_hsequences(dataloader, model, device, resize_shape=(240, 320), top_k_points=1000, pixel_threshold=5,
                               nms_size=15, border_size=15, chunk_sequences=16, batch_size=64):
    """The resize protocol of the HSequences evaluation.  The reference ships its configuration
    (``parse_resize_eval_config``: 240 x 320, ``top_k_points`` 1000, ``pixel_threshold`` 5), its pre-processing
    (``ratio_preserving_resize``, ``adapt_homography_to_preprocessing``), its metric (``compute_resize_repeatability``) and its
    result record (``create_resize_metrics_results``) but no driver loop; the protocol here is:

    * ``dataloader`` has ``.sequences`` and ``get_sequence_data(i)`` returning what ``Resize_HSequences.get_sequence_data``
      returns with ``resize_image=False``: ``im_src_BGR``, ``images_dst_BGR``, ``homographies`` (H_1_k: source -> k-th
      destination, original pixels), ``sequence_name``; images gray or 3-channel uint8 of any size;
    * every image is brought to ``resize_shape`` (``datasets.dataset_utils.ratio_preserving_resize_batch``, one launch per
      chunk) and every homography re-based on the host (``adapt_homography_to_preprocessing``);
    * CHANNEL ORDER: a 3-channel image is taken as BGR (what cv2 reads) and handed to the detector as RGB, as the reference
      converts before detection; a gray image goes as it is (the detector replicates it);
    * each image is detected ONCE (the source is not detected again per destination), ``batch_size`` images per
      ``pipeline.detect_batch_u8`` call -- after the resize all images have one shape --, with ``top_k_points``,
      ``nms_size``, ``border_size``; its rows are (row, col, prob) = (y, x, score);
    * per pair ``compute_resize_repeatability(rows_src, rows_dst, H_resized, resize_shape, resize_shape,
      keep_k_points=top_k_points, distance_thresh=pixel_threshold)``, all pairs of ``chunk_sequences`` sequences in one
      stream-ordered call and ONE device-to-host read per chunk, on which the split-f16 guard is applied as
      ``check_val_hsequences_repeatability`` does (``guard.run_guarded``: a flagged or switched chunk is repeated).

    Returns the ``create_resize_metrics_results`` record: the six lists with one entry per pair in (sequence, destination)
    order (float for the first two, int for the counts), ``sequences`` = the sequence names, ``top_k``, ``pixel_threshold``."""
    device = torch.device(device)
    chunk, batch_size = max(1, int(chunk_sequences)), max(1, int(batch_size))
    names, t = _chunked.run_sequence_chunks(dataloader, model, chunk, RESIZE_RESULT_KEYS, lambda seqs: _resize_chunk(
        seqs, model, device, resize_shape, int(top_k_points), pixel_threshold, nms_size, border_size, batch_size))
    results = create_resize_metrics_results(names, top_k_points, pixel_threshold)
    for k in RESIZE_RESULT_KEYS:
        results[k].extend(map(float if k in ('repeatability', 'localization_err') else int, t[k]))
    return results


# ---- the matching evaluation over a dataset ------------------------------------------------------------------------
_MATCH_FIELDS = ('rep_single_scale', 'rep_multi_scale', 'error_overlap_single_scale', 'error_overlap_multi_scale',
                 'num_points_single_scale', 'num_points_multi_scale', 'candidates_single_scale', 'candidates_multi_scale',
                 'valid', 'mma', 'mma_corr', 'avg_mma', 'num_matches', 'num_mutual_corresp')
_MATCH_COLUMNS = _MATCH_FIELDS + ('kept_src', 'kept_dst')


def _gray_u8(sd_image_u8, image_rgb_norm, device):
    """The uint8 gray image the patches are cut from, on the device: the loader's uint8 image (gray, or BGR as cv2 reads it)
    when it has one, else the normalised RGB image times 255, rounded; colour goes through PIL's ``convert('L')`` arithmetic
    (``ops.rgb_to_gray_u8``), what the demo's ``load_im`` feeds the patch extractor."""
    from .. import ops
    if sd_image_u8 is not None:
        a = _as_rgb_u8(sd_image_u8)
        if a.dtype != np.uint8 or a.shape[:2] != image_rgb_norm.shape[:2]:
            raise ValueError(f"the uint8 image must have the shape of the normalised one: {a.shape} / {image_rgb_norm.shape}")
    else:
        a = np.clip(np.rint(np.asarray(image_rgb_norm, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if t.dim() == 2 else ops.rgb_to_gray_u8(t)


def _matching_chunk(seqs, detector, descriptor, device, nms_size, num_points, border_size, s_mult, th, ths, pixel_threshold,
                    multi_scale, batch_size):
    """Detect and describe the images of some sequences, each once, and evaluate their pairs -> the _MATCH_COLUMNS per pair on
    the host (one read; two when the candidate buffer has to grow); pairs in (sequence, destination) order."""
    images, src_ids, dst_ids, hs, shapes = _chunked.chunk_pairs(seqs)
    if not src_ids:
        return _chunked.Table(_MATCH_COLUMNS)
    u8 = []
    for sd in seqs:
        u8.append(sd.get('im_src_BGR'))
        dst_u8 = sd.get('images_dst_BGR')
        u8.extend(dst_u8 if dst_u8 is not None else [None] * len(sd['images_dst_RGB_norm']))
    rows, count = _chunked.detect_images(images, detector, device, nms_size, num_points, border_size, multi_scale, batch_size)
    desc = _chunked.describe_images([_gray_u8(a, im, device) for a, im in zip(u8, images)], rows, count, descriptor, s_mult,
                                    batch_size)
    s_at, d_at = _chunked.pair_index(src_ids, dst_ids, device)
    args = (rows[s_at], count[s_at], desc[s_at], rows[d_at], count[d_at], desc[d_at], torch.from_numpy(np.stack(hs)).to(device),
            torch.tensor(shapes, dtype=torch.int32, device=device))

    def run(**kw):
        r = evaluate_matching_pairs(*args, th=th, thresholds=ths, pixel_threshold=pixel_threshold, **kw)
        return _chunked.host_table(r, _MATCH_FIELDS, kept_src=r.kept[:, 0], kept_dst=r.kept[:, 1])

    return _chunked.with_edge_retry(run)


@torch.no_grad()
def evaluate_matching_hsequences(dataloader, detector, descriptor, device, num_points=1000, nms_size=15, border_size=15,
                                 s_mult=60, th=0.99, pixel_threshold=5, multi_scale=False, chunk_sequences=16, batch_size=16):
    """The matching evaluation of HSequences (or GoPro): repeatability and matching score of every (source, destination) pair.
    The reference ships the configuration (``--top_k_points``, ``--overlap``, ``--pixel_threshold``) and the result record
    (``create_metrics_results``) but not the loop that fills it; the definitions are DESIGN.md 7h's and
    :func:`evaluate_matching_pairs`'s.

    * ``dataloader`` has ``.sequences`` and ``get_sequence_data(i)`` as ``check_val_hsequences_repeatability`` needs them:
      ``im_src_RGB_norm``, ``images_dst_RGB_norm`` (what the detector sees) and ``h_dst_2_src``; ``sequence_name`` is used
      when present (else ``sequences[i]``).
    * PATCHES are cut from a uint8 gray image: the keys ``im_src_BGR`` / ``images_dst_BGR`` are read when present (gray
      ``[H,W]`` / ``[H,W,1]``, or 3-channel BGR as cv2 reads it; the same size as the normalised image), as the reference's
      ``HSequences.get_sequence_data`` returns them; otherwise ``im_src_RGB_norm * 255`` rounded.  Colour becomes gray with
      PIL's ``convert('L')`` arithmetic on the device, as in the demo.  Every point's patch has scale ``s_mult`` (the demo's
      60), multi-scale points too.
    * ``detector`` is the model, ``descriptor`` a ``HardNet``.  Every image is detected AND described once -- the source is
      not described again for every destination --, images of one shape ``batch_size`` at a time; ``multi_scale`` as in
      ``check_val_hsequences_repeatability``.
    * The pairs of ``chunk_sequences`` sequences are evaluated in one stream-ordered :func:`evaluate_matching_pairs` call with
      thresholds 1..10 and ONE device-to-host read per chunk, on which the split-f16 guard is applied as
      ``check_val_hsequences_repeatability`` does (``guard.run_guarded``: a flagged or switched chunk is repeated).

    Returns ``create_metrics_results(sequence names, num_points, 0.6, pixel_threshold)`` (0.6 = 1 - the ``overlap_err`` of
    ``compute_repeatability``) with one entry per list and pair, in (sequence, destination) order; ``num_features`` holds
    the kept counts (source, destination).  A pair with an empty kept list is skipped, as the repeatability loop skips it
    (``continue``): it has no entry, so that a mean over a list is the mean the loop would have taken."""
    device = torch.device(device)
    chunk, batch_size = max(1, int(chunk_sequences)), max(1, int(batch_size))
    ths, _ = _threshold_index(range(1, 11), pixel_threshold)
    names, t = _chunked.run_sequence_chunks(dataloader, detector, chunk, _MATCH_COLUMNS, lambda seqs: _matching_chunk(
        seqs, detector, descriptor, device, nms_size, int(num_points), border_size, s_mult, th, ths, pixel_threshold,
        multi_scale, batch_size))
    results = create_metrics_results(names, num_points, 0.6, pixel_threshold)
    valid = t['valid'] != 0
    for k in _MATCH_FIELDS:
        if k in results:
            results[k].extend(map(int if k.startswith('num_') else float, t[k][valid]))      # (num_*: the counts)
    results['num_features'].extend((int(a), int(b)) for a, b in zip(t['kept_src'][valid], t['kept_dst'][valid]))
    return results
