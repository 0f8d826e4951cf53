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


def detection_rows(idx, score, count, w):
    """``detect_batch_u8``'s (idx [B,K] flat ``y * w + x``, score [B,K], count [B]) -> rows [B,K,4] float64 (x, y, 1.0, score);
    slots past an image's count are never read by the evaluation."""
    i = idx.to(torch.int64).clamp_(min=0)
    rows = torch.empty(idx.shape + (4,), dtype=torch.float64, device=idx.device)
    rows[..., 0] = i % w
    rows[..., 1] = torch.div(i, w, rounding_mode="floor")
    rows[..., 2] = 1.0
    rows[..., 3] = score
    return rows


def _as_rgb_u8(img):
    """A loader image (``*_BGR``: gray [H,W] / [H,W,1] or BGR [H,W,3] uint8) as the detector's input: gray as it is, colour
    with the channels reversed to RGB (the reference converts BGR to RGB before detection)."""
    a = np.asarray(img)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    return np.ascontiguousarray(a[:, :, ::-1]) if a.ndim == 3 else np.ascontiguousarray(a)


def _resize_chunk(seqs, model, device, resize_shape, top_k, pixel_threshold, nms_size, border_size, batch_size):
    """One chunk of sequences -> [P, 6] float64 on the host (one read), pairs in (sequence, destination) order."""
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
        return np.zeros((0, 6))
    if len({im.ndim for im in images}) != 1:                     # gray and colour in one chunk: gray replicated to 3 channels
        images = [im if im.ndim == 3 else np.repeat(im[:, :, None], 3, axis=2) for im in images]
    batch = dataset_utils.ratio_preserving_resize_batch(images, (th, tw), device)
    rows, counts = [], []
    for b0 in range(0, batch.shape[0], batch_size):
        idx, score, count, _ = detect_batch_u8(model, batch[b0:b0 + batch_size], border_size, nms_size, top_k)
        rows.append(detection_rows(idx, score, count, tw))
        counts.append(count)
    rows, counts = torch.cat(rows), torch.cat(counts)
    i_s = torch.tensor(pair_src, dtype=torch.long, device=rows.device)
    i_d = torch.tensor(pair_dst, dtype=torch.long, device=rows.device)
    shapes = np.tile(np.asarray([th, tw, th, tw], dtype=np.int32), (len(hs), 1))
    r = evaluate_resize_pairs(rows[i_s], counts[i_s], rows[i_d], counts[i_d], np.stack(hs), shapes, top_k, pixel_threshold)
    return torch.stack([r.repeatability, r.localization_err, r.common_src_num.double(), r.common_dst_num.double(),
                        r.rep_src_num.double(), r.rep_dst_num.double()], dim=1).cpu().numpy()      # the one read of the chunk


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
      stream-ordered call and ONE device-to-host read per chunk.  On that read the split-f16 guard is applied as
      ``check_val_hsequences_repeatability`` does: a chunk whose forward was flagged (or during which the checkpoint was
      switched to the fp32 kernels) is repeated.

    Returns the ``create_resize_metrics_results`` record: the six lists with one entry per pair in (sequence, destination)
    order (float for the first two, int for the counts), ``sequences`` = the sequence names, ``top_k``, ``pixel_threshold``."""
    from .test_utils import RESIZE_RESULT_KEYS, create_resize_metrics_results
    device = torch.device(device)
    guard = getattr(model, "fp16_guard_check", None)
    chunk, batch_size = max(1, int(chunk_sequences)), max(1, int(batch_size))
    names, out_rows = [], []
    n_seq = len(dataloader.sequences)
    for c0 in range(0, n_seq, chunk):
        seqs = [dataloader.get_sequence_data(i) for i in range(c0, min(n_seq, c0 + chunk))]
        names.extend(s['sequence_name'] for s in seqs)
        chunk_args = (seqs, model, device, resize_shape, int(top_k_points), pixel_threshold, nms_size, border_size, batch_size)
        on_fp32 = getattr(model, "effective_precision", None) == "fp32"
        out = _resize_chunk(*chunk_args)
        flagged = guard is not None and guard(synchronize=False)     # (the read above has passed every forward of the chunk)
        if flagged or (not on_fp32 and getattr(model, "effective_precision", None) == "fp32"):
            out = _resize_chunk(*chunk_args)
        out_rows.append(out)
    results = create_resize_metrics_results(names, top_k_points, pixel_threshold)
    for r in (np.concatenate(out_rows) if out_rows else np.zeros((0, 6))):
        for j, k in enumerate(RESIZE_RESULT_KEYS):
            results[k].append(float(r[j]) if j < 2 else int(r[j]))
    return results
