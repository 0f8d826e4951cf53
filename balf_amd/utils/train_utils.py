"""The inference / evaluation helpers of /root/reference/balf/utils/train_utils.py with every stage on the GPU.
Training (``train_model``, losses, optimiser; train_utils.py:20-160) is out of scope.

* ``extract_detections`` (train_utils.py:416-454) -- see :mod:`balf_amd.pipeline`.
* ``compute_repeatability_with_maximum_filter`` (train_utils.py:170-196): window-max NMS of both score maps, common-
  region masks (supplied by the caller: the reference builds them with ``cv2.warpPerspective``, which is not rebuilt
  here), top-K points, homography of the destination points, repeatability.
* ``check_val_hsequences_repeatability`` (train_utils.py:308-413): the HSequences validation loop, with every image
  detected once and in batches and all pairs evaluated by the batched core (``benchmark_test.evaluate``).
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


def _evaluate_chunk(seqs, model, device, nms_size, num_points, border_size, multi_scale, batch_size):
    """Detect the images of some sequences and evaluate their pairs -> [P, 10] float64 on the host, one row per pair in
    (sequence, destination) order: rep_s, rep_m, err_s, err_m, possible, valid, found_s, found_m, cand_s, cand_m."""
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
