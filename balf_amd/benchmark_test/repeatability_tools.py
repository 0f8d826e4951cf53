"""``compute_repeatability`` on the GPU: same arguments and result dict as
/root/reference/balf/benchmark_test/repeatability_tools.py:379-490 (callers: train_utils.py:189,257,
dataset_utils.py:332).  The reference's Ns x Nd Python double loop, two dense overlap matrices and their argsorts
become one call into ``balf_repeatability`` (include/balf_hip.h); float64 throughout.  No CPU path.
``compute_repeatability_batch`` is the same for P pairs in one stream-ordered call (``balf_repeatability_batch``).

``apply_nms`` of the same reference module (:19-23) is the window-max NMS: use ``balf_amd.utils.test_utils.apply_nms``.
Its other NMS protocols as score maps -- ``apply_nms_fast`` (:25-79), ``get_nms_score_map_from_score_map`` (:82-100) and
``box_nms`` (:227-255) -- are here under their names, with batched forms that stay on the device (``balf_nms_score_map``).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .. import ops
from .._lib import BalfHipError, Workspace, launch, lib, require_gpu_tensor

MAX_EDGES = 1 << 22


def _device():
    if not torch.cuda.is_available():
        raise BalfHipError("balf_amd has no CPU path: compute_repeatability needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    from .._lib import require_mi355x
    require_mi355x(dev)
    return dev


def compute_repeatability(src_indexes, dst_indexes, overlap_err=0.4, eps=1e-6, dist_match_thresh=3, radious_size=30.):
    src = np.asarray(src_indexes, dtype=np.float64)
    dst = np.asarray(dst_indexes, dtype=np.float64)
    ns, nd = len(src), len(dst)
    points = min(ns, nd)
    found = [0, 0]
    errs = [0.0, 0.0]
    possible = 0
    corr = [np.asarray([]), np.asarray([])]
    if ns > 0 and nd > 0:
        dev = _device()
        s = torch.from_numpy(np.ascontiguousarray(src[:, :3])).to(dev)
        d = torch.from_numpy(np.ascontiguousarray(dst[:, :3])).to(dev)
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        errors = torch.zeros(2, dtype=torch.float64, device=dev)
        cs = torch.empty((points, 2), dtype=torch.int32, device=dev)
        cm = torch.empty((points, 2), dtype=torch.int32, device=dev)
        cap = int(min(ns * nd, MAX_EDGES))
        ws = ops._workspace("repeat", dev, lib().balf_repeatability_workspace_bytes(ns, nd, cap))
        launch("balf_repeatability", dev, s, ns, d, nd, float(overlap_err), float(eps), float(dist_match_thresh),
               float(radious_size), cap, counts, errors, cs, cm, Workspace(ws))
        c = counts.cpu().numpy()
        e = errors.cpu().numpy()
        if c[0] < 0 or c[1] < 0:            # the candidate list of a scale did not fit max_edges (reported by the device)
            raise BalfHipError(f"balf_repeatability: more than {cap} candidate pairs (BALF_ERR_WORKSPACE)")
        found = [int(c[0]), int(c[1])]
        possible = int(c[2])
        errs = [float(e[0]), float(e[1])]
        corr = [cs[:found[0]].cpu().numpy().astype(np.int64) if found[0] else np.asarray([]),
                cm[:found[1]].cpu().numpy().astype(np.int64) if found[1] else np.asarray([])]
    rep_s = (found[0] / np.asarray(points, float)) * 100.0
    rep_m = (found[1] / np.asarray(points, float)) * 100.0
    err_s = 0.0 if found[0] == 0 else errs[0] / float(found[0] + np.finfo(float).eps)
    err_m = 0.0 if found[1] == 0 else errs[1] / float(found[1] + np.finfo(float).eps)
    return {'rep_single_scale': rep_s, 'rep_multi_scale': rep_m, 'num_points_single_scale': found[0],
            'num_points_multi_scale': found[1], 'error_overlap_single_scale': err_s,
            'error_overlap_multi_scale': err_m, 'total_num_points': points,
            'correspondences': corr[0], 'possible_matches': possible, 'correspondences_m': corr[1]}


class RepeatabilityBatch(NamedTuple):
    """Per-pair results of :func:`compute_repeatability_batch`, device tensors ``[P]``: the fields of
    :func:`compute_repeatability`'s dict (float64 / int32) plus the candidate counts of the two scales."""
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


def _counts(c, p, dev, name):
    if not isinstance(c, torch.Tensor) or c.dim() != 1 or c.shape[0] != p or c.device != dev:
        raise BalfHipError(f"{name} must be a [{p}] tensor on {dev}")
    return c if c.dtype == torch.int32 else c.to(torch.int32)


def compute_repeatability_batch(src, ns, dst, nd, overlap_err=0.4, eps=1e-6, dist_match_thresh=3, radious_size=30.,
                                max_edges=None) -> RepeatabilityBatch:
    """:func:`compute_repeatability` for P independent pairs in one stream-ordered call (``balf_repeatability_batch``,
    include/balf_hip.h), bit-identical to it per pair.  ``src`` [P,Ns,C] / ``dst`` [P,Nd,C] float64 rows starting with
    (x, y, radius) on the GPU, ``ns`` / ``nd`` [P] int32 on the GPU (rows past a pair's count are ignored).  Returns device
    tensors and reads nothing back: capturable with ``torch.cuda.graph``.  A pair with a zero count gets rep NaN (the
    reference's 0 / 0.0) and is what the reference's caller skips.  ``max_edges`` bounds the candidate pairs of each scale
    summed over all pairs (default: ``min(P Ns Nd, MAX_EDGES)``); a pair whose candidates do not fit reports
    ``num_points_* = -1`` with NaN rep / error, and ``candidates_*`` says what it needed."""
    for t, name in ((src, "src"), (dst, "dst")):
        require_gpu_tensor(t, name)
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] < 3:
            raise BalfHipError(f"{name} must be a [P,N,C>=3] float64 tensor")
    p, ns_max, nd_max = src.shape[0], src.shape[1], dst.shape[1]
    if dst.shape[0] != p or p == 0:
        raise BalfHipError(f"src and dst must hold the same number (> 0) of pairs, got {p} and {dst.shape[0]}")
    dev = src.device
    ns, nd = _counts(ns, p, dev, "ns"), _counts(nd, p, dev, "nd")
    if ns.stride(0) != nd.stride(0):
        ns, nd = ns.contiguous(), nd.contiguous()
    if max_edges is None:
        max_edges = max(1, min(p * ns_max * nd_max, MAX_EDGES))
    rep = torch.empty((p, 4), dtype=torch.float64, device=dev)
    cnt = torch.empty((p, 6), dtype=torch.int32, device=dev)
    nbytes = lib().balf_repeatability_batch_workspace_bytes(p, ns_max, nd_max, int(max_edges))
    if nbytes == 0:
        raise BalfHipError(f"balf_repeatability_batch: unsupported sizes P={p}, Ns={ns_max}, Nd={nd_max}, max_edges={max_edges}")
    ws = ops._workspace("repeat_batch", dev, nbytes)
    launch("balf_repeatability_batch", dev, src, ns, ns_max, src.shape[2], dst, nd, nd_max, dst.shape[2], ns.stride(0), p,
           float(overlap_err), float(eps), float(dist_match_thresh), float(radious_size), int(max_edges), rep, cnt, Workspace(ws))
    return RepeatabilityBatch(rep[:, 0], rep[:, 1], rep[:, 2], rep[:, 3], cnt[:, 0], cnt[:, 1], cnt[:, 2], cnt[:, 3],
                              cnt[:, 4], cnt[:, 5])


# ---- NMS score maps (reference repeatability_tools.py:25-100, 227-255) --------------------------------------------------------
def box_nms_batch(prob, size=4, iou=0.1, min_prob=0.015, keep_top_k=-1):
    """:func:`box_nms` of every map of ``prob`` [B,H,W] (float32, on the GPU) in one stream-ordered call -> [B,H,W] on the same
    device.  Nothing is read back."""
    return ops.nms_score_map(prob, "box", conf_thresh=min_prob, size=size, iou=iou, keep_top_k=keep_top_k)[0]


def nms_fast_score_map_batch(prob, dist_thresh, conf_thresh=0.015):
    """:func:`apply_nms_fast` of every map of ``prob`` [B,H,W] (float32, on the GPU) in one stream-ordered call -> [B,H,W] on
    the same device.  Nothing is read back."""
    return ops.nms_score_map(prob, "greedy", conf_thresh=conf_thresh, dist_thresh=dist_thresh)[0]


def box_nms(prob, size=4, iou=0.1, min_prob=0.015, keep_top_k=-1):
    """The reference's ``box_nms`` (repeatability_tools.py:227-255) on the GPU: ``prob`` a [1,H,W] float32 tensor -> the [1,H,W]
    map of the boxes that torchvision's NMS keeps (each pixel >= ``min_prob`` is a ``size x size`` box around itself), on the
    input's device.  The IoU test is a footprint of pixel offsets computed once on the host (``ops.box_footprint``: ``2 * size``
    must be a positive integer, ``size <= 17``, ``0 <= iou < 1``, ``min_prob > 0``; ValueError otherwise).  Among equal scores,
    also at the ``keep_top_k`` cut, the lower raster index comes first."""
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3 or prob.shape[0] != 1:
        raise BalfHipError("prob must be a [1,H,W] tensor")
    if not prob.is_cuda:
        raise BalfHipError(f"balf_amd has no CPU path: box_nms needs prob on the GPU (got device {prob.device})")
    return box_nms_batch(prob, size, iou, min_prob, keep_top_k)


def _score_map_on_gpu(score_map, what):
    m = np.ascontiguousarray(score_map, dtype=np.float32)
    if m.ndim != 2:
        raise ValueError(f"{what}: score map must be [H, W]")
    if not torch.cuda.is_available():
        raise BalfHipError(f"balf_amd has no CPU path: {what} needs the GPU")
    return torch.from_numpy(m).to(_device()).unsqueeze(0)


def apply_nms_fast(score_map, dist_thresh, conf_thresh=0.015):
    """The reference's ``apply_nms_fast`` (repeatability_tools.py:25-79) on the GPU: NumPy [H,W] map in, NumPy float32 map out.
    The greedy ``(2 dist_thresh + 1)^2`` sweep over ALL pixels in descending score order, survivors >= ``conf_thresh`` kept: a
    pixel below the threshold only suppresses pixels that are dropped anyway, so this is the greedy NMS of the candidates
    >= ``conf_thresh``.  1 <= ``dist_thresh`` <= 16, ``conf_thresh`` > 0; equal scores: the lower raster index
    first."""
    return nms_fast_score_map_batch(_score_map_on_gpu(score_map, "apply_nms_fast"), dist_thresh, conf_thresh)[0].cpu().numpy()


def get_nms_score_map_from_score_map(heatmap, conf_thresh=0.015, nms_size=15):
    """The reference's function of this name (repeatability_tools.py:82-100): the same map as
    ``apply_nms_fast(heatmap, nms_size, conf_thresh)``."""
    t = _score_map_on_gpu(heatmap, "get_nms_score_map_from_score_map")
    return nms_fast_score_map_batch(t, nms_size, conf_thresh)[0].cpu().numpy()


def check_common_points(kpts, mask):
    """Indices of the key points (rows ``[y, x, ...]``) that fall inside ``mask`` (repeatability_tools.py:8-13; index
    bookkeeping on the host, like the reference: note its off-by-one ``mask[round(y) - 1, round(x) - 1]``)."""
    kpts = np.asarray(kpts)
    if len(kpts) == 0:
        return np.asarray([])
    r = np.rint(kpts[:, :2]).astype(np.int64) - 1
    return np.flatnonzero(np.asarray(mask)[r[:, 0], r[:, 1]] != 0)


def select_top_k(kpts, k=1000):
    """Indices of the ``k`` highest-scoring rows (score in column 3; repeatability_tools.py:15-17)."""
    return np.argsort(-1 * np.asarray(kpts)[:, 3])[:k]


# ---- the resize protocol (reference repeatability_tools.py:516-614) -----------------------------------------------------------
class ResizeRepeatabilityBatch(NamedTuple):
    """Per-pair results of :func:`compute_resize_repeatability_batch`, device tensors ``[P]``: the fields of
    :func:`compute_resize_repeatability`'s dict (float64 / int32)."""
    repeatability: torch.Tensor
    localization_err: torch.Tensor
    common_src_num: torch.Tensor
    common_dst_num: torch.Tensor
    rep_src_num: torch.Tensor
    rep_dst_num: torch.Tensor


def _host_or_device(t, dev, dtype, shapes_ok, name):
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype={torch.float64: np.float64, torch.int32: np.int32}[dtype]))
    if tuple(t.shape) not in shapes_ok:
        raise BalfHipError(f"{name} must have shape {' or '.join(map(str, shapes_ok))}, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=dtype).contiguous()


def compute_resize_repeatability_batch(src, ns, dst, nd, h, shapes, keep_k_points=1000, distance_thresh=5, h_inv=None,
                                       order="rcp") -> ResizeRepeatabilityBatch:
    """:func:`compute_resize_repeatability` for P independent pairs in one stream-ordered call
    (``balf_resize_repeatability_batch``, include/balf_hip.h), equal to it per pair bit for bit.  ``src`` [P,Ns,C] / ``dst``
    [P,Nd,C] float64 rows on the GPU -- ``order='rcp'``: (row, col, prob), the reference's; ``order='xyrs'``: (x, y, radius,
    score), this library's detector rows --, ``ns`` / ``nd`` [P] int32 on the GPU (rows past a count are never read), ``h``
    [P,3,3] source -> destination in (x, y), ``shapes`` [P,4] = (h_src, w_src, h_dst, w_dst).  ``h_inv`` None: ``h`` is a host
    array and ``np.linalg.inv`` runs on the host, as in the reference (two small uploads: not capturable); with ``h`` and
    ``h_inv`` both device tensors nothing leaves the device and the call can be captured with ``torch.cuda.graph``.
    Tie rule of ``select_k_best``: higher prob first, then the lower row index.  No input is written."""
    require_gpu_tensor(src, "src")
    dev, p = src.device, src.shape[0]
    if h_inv is None:
        if isinstance(h, torch.Tensor):
            h = h.detach().cpu().numpy()
        h = np.asarray(h).reshape(-1, 3, 3)
        h_inv = np.linalg.inv(h)
    h = _host_or_device(h, dev, torch.float64, ((p, 3, 3), (p, 9)), "h")
    h_inv = _host_or_device(h_inv, dev, torch.float64, ((p, 3, 3), (p, 9)), "h_inv")
    shapes = _host_or_device(shapes, dev, torch.int32, ((p, 4),), "shapes")
    ns, nd = _counts(ns, p, dev, "ns").contiguous(), _counts(nd, p, dev, "nd").contiguous()
    rep, cnt = ops.resize_repeatability_batch(src, ns, dst, nd, h, h_inv, shapes, keep_k_points, distance_thresh, order)
    return ResizeRepeatabilityBatch(rep[:, 0], rep[:, 1], cnt[:, 0], cnt[:, 1], cnt[:, 2], cnt[:, 3])


def compute_resize_repeatability(keypoints, warped_keypoints, h, shape_src, shape_dst, keep_k_points=1000, distance_thresh=5):
    """The reference's resize-protocol metric (repeatability_tools.py:516-614) on the GPU: same arguments, same dict, same
    value types.  ``keypoints`` [N,3] / ``warped_keypoints`` [M,3] rows (row, col, prob) of the source / destination image,
    ``h`` the 3x3 homography source -> destination in (x, y) (``np.linalg.inv(h)`` is taken on the host, as there).

    Two deliberate differences: among rows of EQUAL prob at the ``keep_k_points`` cut the lower row index is kept (the
    reference's ``argsort`` is unstable there); and ``keypoints`` is NOT overwritten -- the reference writes the warped
    coordinates into the caller's array, so that a source array used for a second destination is already warped."""
    kp = np.asarray(keypoints, dtype=np.float64).reshape(-1, 3)
    wkp = np.asarray(warped_keypoints, dtype=np.float64).reshape(-1, 3)
    h = np.asarray(h).reshape(3, 3)
    dev = _device()
    s = torch.from_numpy(np.ascontiguousarray(kp)).to(dev)[None]
    d = torch.from_numpy(np.ascontiguousarray(wkp)).to(dev)[None]
    ns = torch.tensor([len(kp)], dtype=torch.int32, device=dev)
    nd = torch.tensor([len(wkp)], dtype=torch.int32, device=dev)
    shapes = np.asarray([[shape_src[0], shape_src[1], shape_dst[0], shape_dst[1]]], dtype=np.int32)
    r = compute_resize_repeatability_batch(s, ns, d, nd, h[None], shapes, keep_k_points, distance_thresh)
    rep, err = float(r.repeatability[0]), float(r.localization_err[0])
    n1, n2, c1, c2 = (int(t[0]) for t in (r.common_src_num, r.common_dst_num, r.rep_src_num, r.rep_dst_num))
    # the reference's value types: NumPy scalars where it computed with NumPy, Python numbers where it did not
    found = c1 + c2 > 0
    return {'repeatability': np.float64(rep) if found else 0., 'localization_err': np.float64(err) if found else -1,
            'common_src_num': n1, 'common_dst_num': n2,
            'rep_src_num': np.int64(c1) if n2 != 0 else 0, 'rep_dst_num': np.int64(c2) if n1 != 0 else 0}
