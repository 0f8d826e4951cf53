"""The inference / evaluation helpers of /root/reference/balf/utils/train_utils.py with every stage on the GPU.
Training (``train_model``, losses, optimiser; train_utils.py:20-160) is out of scope.

* ``extract_detections`` (train_utils.py:416-454) -- see :mod:`balf_amd.pipeline`.
* ``compute_repeatability_with_maximum_filter`` (train_utils.py:170-196): window-max NMS of both score maps, common-
  region masks (supplied by the caller: the reference builds them with ``cv2.warpPerspective``, which is not rebuilt
  here), top-K points, homography of the destination points, repeatability.
* ``check_val_hsequences_repeatability`` (train_utils.py:308-413): the HSequences validation loop, with every image
  detected once and in batches and all pairs evaluated by the batched core (``benchmark_test.evaluate``).
* ``check_val_repeatability`` (train_utils.py:205-306): the per-epoch validation on synthetic-homography pairs that the
  reference selects checkpoints by (train.py:87,113), pairs forwarded in batches and both of its evaluations (greedy NMS
  and window NMS) run by the batched core from the same forward.  Its tensorboard logging -- and with it
  ``prob_to_score_maps_tensor_batch`` / ``apply_nms_fast`` (train_utils.py:162-168) -- is not ported.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from .. import multiscale
from ..benchmark_test import evaluate, geometry_tools, repeatability_tools
from ..pipeline import detect_batch, extract_detections, pad_image_on_device  # noqa: F401
from . import test_utils


def compute_repeatability_with_maximum_filter(src_scores_np, dst_scores_np, homography, mask_src, mask_dst, nms_size,
                                              num_points):
    src_scores_common_nms = np.multiply(test_utils.apply_nms(src_scores_np, nms_size), mask_src)
    dst_scores_common_nms = np.multiply(test_utils.apply_nms(dst_scores_np, nms_size), mask_dst)
    src_pts_nms = test_utils.get_point_coordinates(src_scores_common_nms, num_points=num_points, order_coord='xysr')
    dst_pts_nms = test_utils.get_point_coordinates(dst_scores_common_nms, num_points=num_points, order_coord='xysr')
    dst_to_src_pts_nms = geometry_tools.apply_homography_to_points(dst_pts_nms, homography)
    r = repeatability_tools.compute_repeatability(src_pts_nms, dst_to_src_pts_nms)
    return ([r['rep_single_scale']], [r['rep_multi_scale']], [r['error_overlap_single_scale']],
            [r['error_overlap_multi_scale']], [r['possible_matches']])



def _detect_images(images, model, device, nms_size, num_points, border_size, multi_scale, batch_size):
    """[H,W,3] float images on the host -> (rows [I,K,4] float64, count [I] int32) on the device: rows (x, y, radius, score)
    as ``extract_detections`` (radius 1.0) or ``extract_multiscale_detections`` returns them, rows past the count unused.
    Images of one shape go through the detector together, ``batch_size`` at a time (detection is batch-invariant)."""
    rows = torch.zeros((len(images), num_points, 4), dtype=torch.float64, device=device)
    count = torch.zeros((len(images),), dtype=torch.int32, device=device)
    groups = OrderedDict()
    for i, im in enumerate(images):
        groups.setdefault((im.shape[0], im.shape[1]), []).append(i)
    for (h, w), ids in groups.items():
        for b0 in range(0, len(ids), batch_size):
            sel = ids[b0:b0 + batch_size]
            at = torch.tensor(sel, dtype=torch.long, device=device)
            if multi_scale:
                x = torch.stack([torch.from_numpy(np.ascontiguousarray(images[i] if images[i].dtype in (np.float64, np.float32, np.float16)
                                                                       else images[i].astype(np.float64))).to(device)
                                 for i in sel]).to(torch.float32)
                pts, cnt = multiscale.detect_batch_multiscale(model, x, num_points=num_points, border_size=border_size,
                                                              nms_size=nms_size)
                rows[at] = pts
            else:
                x = torch.cat([pad_image_on_device(images[i], device) for i in sel])
                idx, score, cnt, _ = detect_batch(model, x, h, w, border_size, nms_size, num_points)
                idx = idx.to(torch.int64)
                rows[at] = torch.stack([(idx % w).double(), (idx // w).double(), torch.ones_like(score, dtype=torch.float64),
                                        score.double()], dim=2)
            count[at] = cnt
    return rows, count


def _chunk_pairs(seqs):
    """The images of some sequences, each once, and their pairs in (sequence, destination) order -> (images, src_ids, dst_ids,
    hs, shapes): pair k is images[src_ids[k]] / images[dst_ids[k]] with h_dst_2_src hs[k] and shapes[k] = (h_src, w_src, h_dst,
    w_dst)."""
    images, src_ids, dst_ids, hs, shapes = [], [], [], [], []
    for sd in seqs:
        src = sd['im_src_RGB_norm']
        si = len(images)
        images.append(src)
        for k, im in enumerate(sd['images_dst_RGB_norm']):
            src_ids.append(si)
            dst_ids.append(len(images))
            images.append(im)
            hs.append(np.asarray(sd['h_dst_2_src'][k], dtype=np.float64).reshape(3, 3))
            shapes.append((src.shape[0], src.shape[1], im.shape[0], im.shape[1]))
    return images, src_ids, dst_ids, hs, shapes


def _evaluate_chunk(seqs, model, device, nms_size, num_points, border_size, multi_scale, batch_size):
    """Detect the images of some sequences and evaluate their pairs -> [P, 10] float64 on the host, one row per pair in
    (sequence, destination) order: rep_s, rep_m, err_s, err_m, possible, valid, found_s, found_m, cand_s, cand_m."""
    images, src_ids, dst_ids, hs, shapes = _chunk_pairs(seqs)
    if not src_ids:
        return np.zeros((0, 10))
    rows, count = _detect_images(images, model, device, nms_size, num_points, border_size, multi_scale, batch_size)
    s_at = torch.tensor(src_ids, dtype=torch.long, device=device)
    d_at = torch.tensor(dst_ids, dtype=torch.long, device=device)
    args = (rows[s_at], count[s_at], rows[d_at], count[d_at], torch.from_numpy(np.stack(hs)).to(device),
            torch.tensor(shapes, dtype=torch.int32, device=device))

    def run(**kw):
        r = evaluate.evaluate_pairs(*args, **kw)
        return torch.stack([r.rep_single_scale, r.rep_multi_scale, r.error_overlap_single_scale, r.error_overlap_multi_scale,
                            r.possible_matches.double(), r.valid.double(), r.num_points_single_scale.double(),
                            r.num_points_multi_scale.double(), r.candidates_single_scale.double(),
                            r.candidates_multi_scale.double()], dim=1).cpu().numpy()

    out = run()                         # the one device-to-host read of the chunk
    if (out[:, 6:8] < 0).any():         # some pair's candidates did not fit the default buffer: size it from the totals
        out = run(max_edges=int(max(out[:, 8].sum(), out[:, 9].sum(), 1)))
    return out


@torch.no_grad()
def check_val_hsequences_repeatability(dataloader, model, device, tb_log, cur_epoch, cell_size=8, nms_size=15, num_points=25,
                                       border_size=15, multi_scale=False, chunk_sequences=16, batch_size=16):
    """The reference's HSequences validation (train_utils.py:308-413): same arguments, same five means (rep_s, rep_m,
    error_overlap_s, error_overlap_m, possible_matches over the pairs where both images keep points in the common region),
    bit-identical to its loop.  ``dataloader`` provides ``.sequences`` and ``get_sequence_data(i)`` with
    ``im_src_RGB_norm``, ``images_dst_RGB_norm`` and ``h_dst_2_src``.

    Instead of detecting the source image again for every destination, each image is detected once, images of one shape
    ``batch_size`` at a time (detection is deterministic and batch-invariant), and the pairs of ``chunk_sequences``
    sequences are evaluated together on the device (``benchmark_test.evaluate.evaluate_pairs``); the per-pair results are
    read once per chunk.  On that read the split-f16 guard is applied as ``extract_detections`` does: a chunk whose forward
    was flagged is repeated (on the fp32 kernels).  ``multi_scale=True`` detects with ``multiscale.detect_batch_multiscale``
    (``pyramid_plan`` defaults; ``num_points`` / ``nms_size`` / ``border_size`` as given), the multi-scale HSequences
    protocol, equal to the same loop over ``extract_multiscale_detections``.  ``tb_log`` must be None: the reference's
    image logging is not ported.  ``cell_size`` and ``cur_epoch`` are unused, as in the reference."""
    if tb_log is not None:
        raise NotImplementedError("check_val_hsequences_repeatability: tensorboard image logging is not ported; pass tb_log=None")
    device = torch.device(device)
    guard = getattr(model, "fp16_guard_check", None)
    rep_s, rep_m, error_overlap_s, error_overlap_m, possible_matches = [], [], [], [], []
    n_seq = len(dataloader.sequences)
    for c0 in range(0, n_seq, max(1, int(chunk_sequences))):
        seqs = [dataloader.get_sequence_data(i) for i in range(c0, min(n_seq, c0 + max(1, int(chunk_sequences))))]
        chunk_args = (seqs, model, device, nms_size, num_points, border_size, multi_scale, int(batch_size))
        out = _evaluate_chunk(*chunk_args)
        if guard is not None and guard(synchronize=False):     # (the read above has passed every forward of the chunk)
            out = _evaluate_chunk(*chunk_args)
        for r in out:
            if r[5] == 0:
                continue
            rep_s.append(float(r[0]))
            rep_m.append(float(r[1]))
            error_overlap_s.append(float(r[2]))
            error_overlap_m.append(float(r[3]))
            possible_matches.append(int(r[4]))
    return np.asarray(rep_s).mean(), np.asarray(rep_m).mean(), np.asarray(error_overlap_s).mean(), \
        np.asarray(error_overlap_m).mean(), np.asarray(possible_matches).mean()


_VAL_CONF_THRESH = 0.015      # get_nms_score_map_from_score_map(..., conf_thresh=0.015), train_utils.py:242-243


def _evaluate_val_chunk(pairs, model, device, nms_size, num_points, batch_size, max_edges=None):
    """``pairs``: (image_src [3,Hs,Ws], image_dst [3,Hd,Wd], h_dst_2_src [3,3]) tensors.  Forward them (pairs of one shape
    ``batch_size`` at a time) and evaluate both legs from that forward -> [P, 2, 9] float64 on the host (leg 0 greedy, leg 1
    window): rep_s, rep_m, err_s, err_m, possible, found_s, found_m, cand_s, cand_m."""
    out = torch.zeros((len(pairs), 2, 9), dtype=torch.float64, device=device)
    groups = OrderedDict()
    for i, (src, dst, _) in enumerate(pairs):
        groups.setdefault((tuple(src.shape), tuple(dst.shape)), []).append(i)
    kw = {} if max_edges is None else {"max_edges": int(max_edges)}
    for ids in groups.values():
        for b0 in range(0, len(ids), batch_size):
            sel = ids[b0:b0 + batch_size]
            prob_src = model(torch.stack([pairs[i][0] for i in sel]).to(device), want_logits=False)["prob"]
            prob_dst = model(torch.stack([pairs[i][1] for i in sel]).to(device), want_logits=False)["prob"]
            h = torch.stack([pairs[i][2].reshape(3, 3) for i in sel]).to(device=device, dtype=torch.float64)
            at = torch.tensor(sel, dtype=torch.long, device=device)
            for leg_id, leg in enumerate(("greedy", "window")):
                r = evaluate.evaluate_val_pairs(prob_src, prob_dst, h, nms_size, num_points, leg=leg,
                                                conf_thresh=_VAL_CONF_THRESH, **kw)
                out[at, leg_id] = torch.stack([r.rep_single_scale, r.rep_multi_scale, r.error_overlap_single_scale,
                                               r.error_overlap_multi_scale, r.possible_matches.double(),
                                               r.num_points_single_scale.double(), r.num_points_multi_scale.double(),
                                               r.candidates_single_scale.double(), r.candidates_multi_scale.double()], dim=1)
    return out.cpu().numpy()            # the one device-to-host read of the chunk


def _val_chunk(*args):
    out = _evaluate_val_chunk(*args)
    if (out[:, :, 5:7] < 0).any():      # some pair's candidates did not fit the default buffer: size it from the totals
        out = _evaluate_val_chunk(*args, max_edges=int(max(out[:, :, 7].sum(axis=0).max(), out[:, :, 8].sum(axis=0).max(), 1)))
    return out


@torch.no_grad()
def check_val_repeatability(dataloader, model, device, tb_log, cur_epoch, cell_size=8, nms_size=15, num_points=25,
                            chunk_pairs=64, batch_size=16):
    """The reference's per-epoch validation (train_utils.py:205-306): same arguments, same ten return values.
    ``dataloader`` yields 6-tuples ``(images_src, images_dst, heatmap_src, heatmap_dst, h_src_2_dst, h_dst_2_src)`` of
    batched tensors; images ``[B,3,H,W]`` with H, W multiples of 64 (no padding, no crop, as in the reference).  Two
    properties of the reference's loop are reproduced on purpose:

    * only ELEMENT 0 of every loader batch is evaluated (:232-243); elements 1.. are never looked at (the reference
      forwards them and drops the result; here they are not even forwarded -- detection is batch-invariant);
    * the first five values (rep_s, rep_m, error_overlap_s, error_overlap_m, possible_matches) are means over all evaluated
      pairs of the greedy-NMS leg, but the five ``_nms`` values are NOT accumulated: the reference re-creates their lists in
      every iteration (``compute_repeatability_with_maximum_filter`` returns fresh one-element lists), so they are the
      window-NMS values of the LAST pair alone.

    Per pair and leg: NMS of both score maps (greedy: candidates >= 0.015, ``nms_fast`` with ``dist_thresh = nms_size``;
    window: ``apply_nms``), times the common-region mask, the ``num_points`` best in raster order, homography of the
    destination points, repeatability -- ``benchmark_test.evaluate.evaluate_val_pairs``, both legs from the SAME forward.
    Pairs of one shape are forwarded ``batch_size`` at a time and the results of ``chunk_pairs`` pairs are read with one
    device-to-host copy.  On that read the split-f16 guard is applied as ``check_val_hsequences_repeatability`` does (a
    chunk whose forward was flagged, or during which the checkpoint was switched to the fp32 kernels, is repeated on them), and a chunk whose candidate pairs did not fit the
    default buffer is repeated with a buffer sized from the reported totals.  ``h_dst_2_src`` is used as float64.
    ``tb_log`` must be None: the reference's image logging is not ported.  ``cell_size`` and ``cur_epoch``
    are unused, as in the reference.  An empty loader raises ValueError (the reference fails with a NameError)."""
    if tb_log is not None:
        raise NotImplementedError("check_val_repeatability: tensorboard image logging is not ported; pass tb_log=None")
    device = torch.device(device)
    guard = getattr(model, "fp16_guard_check", None)
    chunk_pairs, batch_size = max(1, int(chunk_pairs)), max(1, int(batch_size))
    rows, pairs = [], []

    def flush():
        args = (list(pairs), model, device, nms_size, num_points, batch_size)
        on_fp32 = getattr(model, "effective_precision", None) == "fp32"
        out = _val_chunk(*args)
        # (the read above has passed every forward of the chunk.)  A chunk runs several forwards, and a later one may already
        # have looked at an earlier one's status block and switched the checkpoint to the fp32 kernels, after the flagged score
        # map went into the selection: a switch during the chunk repeats it just as a flag found now does.
        flagged = guard is not None and guard(synchronize=False)
        if flagged or (not on_fp32 and getattr(model, "effective_precision", None) == "fp32"):
            out = _val_chunk(*args)
        rows.append(out)
        pairs.clear()

    for batch in dataloader:
        images_src, images_dst, _, _, _, h_dst_2_src = batch
        pairs.append((images_src[0], images_dst[0], h_dst_2_src[0]))
        if len(pairs) == chunk_pairs:
            flush()
    if pairs:
        flush()
    if not rows:
        raise ValueError("check_val_repeatability: the dataloader is empty")
    out = np.concatenate(rows)
    greedy, last = np.ascontiguousarray(out[:, 0].T), out[-1, 1]          # (contiguous: the summation order of a 1-D array)
    return (greedy[0].mean(), greedy[1].mean(), greedy[2].mean(), greedy[3].mean(), greedy[4].mean(),
            np.asarray([last[0]]).mean(), np.asarray([last[1]]).mean(), np.asarray([last[2]]).mean(),
            np.asarray([last[3]]).mean(), np.asarray([last[4]]).mean())
