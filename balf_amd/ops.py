"""Thin torch-tensor wrappers over the C ABI (device memory and streams are PyTorch's; the compute
is the HIP library's).  Every function requires CUDA tensors and raises otherwise."""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .arch import padded_hw
from ._lib import BalfHipError, Workspace, check, launch, lib, on_device, require_gpu_tensor

_workspaces: Dict[Tuple[str, int, int], torch.Tensor] = {}      # insertion order = least recently used first
_MAX_STREAMS_PER_TAG = 2        # the forward workspace of 8 x 1088x1920 is ~7 GB: a process that keeps creating streams
                                # must not pin one per stream it ever used


def _workspace(tag: str, device, nbytes: int) -> torch.Tensor:
    """Caller-owned scratch (the library never allocates), cached per (purpose, device, STREAM) and grown on demand.
    Kernels of one stream run in order, so one buffer per stream is race-free; two streams (or two models driven from
    two streams) get two buffers.  A buffer that is replaced by a larger one -- or evicted: at most _MAX_STREAMS_PER_TAG
    streams per (purpose, device) keep theirs, least recently used first out -- is handed back to the caching allocator,
    which re-issues it in the order of the stream it was allocated and last used on.  (A raw stream handle may be
    recycled for a new stream after its owner is destroyed; the entry it then finds was last used on the destroyed
    stream, whose work the runtime completes before the handle is reused.)"""
    dev_index = device.index if device.index is not None else torch.cuda.current_device()
    key = (tag, dev_index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = None                                            # drop the smaller buffer before asking for the larger one
        with torch.cuda.device(device):
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        same = [k for k in _workspaces if k[0] == tag and k[1] == dev_index]
        for k in same[:max(0, len(same) - (_MAX_STREAMS_PER_TAG - 1))]:
            del _workspaces[k]
    _workspaces[key] = ws                                    # (re)inserted last: most recently used
    return ws


def release_workspaces() -> None:
    _workspaces.clear()


def window_nms(score: torch.Tensor, border: int, nms_size: int) -> torch.Tensor:
    """[B,H,W] fp32 -> dense apply_nms(remove_borders(score, border), nms_size)
    (/root/reference/balf/utils/test_utils.py:34-54)."""
    require_gpu_tensor(score, "score")
    if score.dtype != torch.float32 or score.dim() != 3:
        raise BalfHipError("score must be a [B,H,W] float32 tensor")
    out = torch.empty_like(score)
    b, h, w = score.shape
    launch("balf_window_nms", score.device, score, b, h, w, int(border), int(nms_size), out)
    return out


def nms_topk(prob: torch.Tensor, crop_y: int, crop_x: int, h: int, w: int, border: int, nms_size: int,
             k: int, threshold: float = -1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[B,Hp,Wp] fp32 score maps -> (idx [B,K] int32, score [B,K] fp32, count [B] int32); see
    balf_nms_topk in include/balf_hip.h.  ``k > h*w`` raises IndexError like the reference
    (/root/reference/balf/utils/test_utils.py:83).  ``threshold > 0`` selects by that value instead of the K-th
    largest score (balf_nms_threshold; ``threshold != -1`` of find_index_higher_scores, test_utils.py:91-95)."""
    require_gpu_tensor(prob, "prob")
    if prob.dtype != torch.float32 or prob.dim() != 3:
        raise BalfHipError("prob must be a [B,Hp,Wp] float32 tensor")
    if k > h * w:
        raise IndexError(f"index {k - 1} is out of bounds for axis 0 with size {h * w}")
    b, hp, wp = prob.shape
    dev = prob.device
    idx = torch.empty((b, k), dtype=torch.int32, device=dev)
    score = torch.empty((b, k), dtype=torch.float32, device=dev)
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    nbytes = lib().balf_nms_topk_workspace_bytes(b, h, w, k)
    ws = _workspace("nms", dev, nbytes)
    if threshold == -1:
        launch("balf_nms_topk", dev, prob, b, hp, wp, int(crop_y), int(crop_x), int(h), int(w), int(border), int(nms_size), int(k),
               idx, score, count, Workspace(ws))
    else:
        launch("balf_nms_threshold", dev, prob, b, hp, wp, int(crop_y), int(crop_x), int(h), int(w), int(border), int(nms_size),
               float(threshold), int(k), idx, score, count, Workspace(ws))
    return idx, score, count


def greedy_nms(prob: torch.Tensor, crop_y: int, crop_x: int, h: int, w: int, border: int, conf_thresh: float,
               dist_thresh: int, k: int, subpixel_patch: int = 0):
    """Greedy NMS of the demo path (balf_greedy_nms in include/balf_hip.h).  Returns
    (idx [B,K] int32, score [B,K], xy [B,K,2] or None, count [B], total [B])."""
    require_gpu_tensor(prob, "prob")
    if prob.dtype != torch.float32 or prob.dim() != 3:
        raise BalfHipError("prob must be a [B,Hp,Wp] float32 tensor")
    b, hp, wp = prob.shape
    dev = prob.device
    idx = torch.empty((b, k), dtype=torch.int32, device=dev)
    score = torch.empty((b, k), dtype=torch.float32, device=dev)
    xy = torch.empty((b, k, 2), dtype=torch.float32, device=dev) if subpixel_patch > 0 else None
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    total = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = _workspace("greedy", dev, lib().balf_greedy_nms_workspace_bytes(b, h, w, k))
    launch("balf_greedy_nms", dev, prob, b, hp, wp, int(crop_y), int(crop_x), int(h), int(w), int(border), float(conf_thresh),
           int(dist_thresh), int(k), int(subpixel_patch), idx, score, xy, count, total, Workspace(ws))
    return idx, score, xy, count, total


# ---- NMS score maps (benchmark_test/repeatability_tools.py and utils/train_utils.py drive these) -----------------------------
NMS_MAP_PROTOCOLS = {"greedy": _lib.NMS_MAP_GREEDY, "box": _lib.NMS_MAP_BOX}


def box_footprint(size, iou) -> Tuple[int, Tuple[int, ...]]:
    """The suppression footprint of ``box_nms(size=size, iou=iou)`` -> ``(radius, rows)``: ``rows[dr + radius]`` has bit
    ``dc + radius`` set iff two ``size x size`` boxes whose centres lie ``(dr, dc)`` apart have IoU > ``iou``, with the float32
    operations of the reference's ``box_iou`` (balf/benchmark_test/repeatability_tools.py:271-291 there) and its
    comparison with ``float32(iou)``.  ``2 * size`` must be a positive integer: every box coordinate is then exact in float32
    and the IoU depends on the offset alone.  ``radius = ceil(size) - 1`` (boxes further apart do not overlap) must not exceed
    16; ``0 <= iou < 1``.  ValueError otherwise."""
    size, iou = float(size), float(iou)
    if not (size > 0.0) or 2.0 * size != np.floor(2.0 * size):
        raise ValueError(f"box_footprint: 2 * size must be a positive integer, got size={size}")
    if not (0.0 <= iou < 1.0):
        raise ValueError(f"box_footprint: iou must lie in [0, 1), got {iou}")
    radius = int(np.ceil(size)) - 1
    if radius > _lib.NMS_MAP_MAX_RADIUS:
        raise ValueError(f"box_footprint: size={size} gives radius {radius}, above {_lib.NMS_MAP_MAX_RADIUS}")
    f32 = np.float32
    half = f32(size / 2.0)
    d = np.arange(-radius, radius + 1, dtype=np.float32)
    lo, hi = d - half, d + half                                      # the moved box along one axis; the other one is (-half, half)
    side = np.maximum(np.minimum(hi, half) - np.maximum(lo, -half), f32(0)).astype(np.float32)
    inter = (side[:, None] * side[None, :]).astype(np.float32)
    area = f32((half - -half) * (half - -half))
    with np.errstate(invalid="ignore", divide="ignore"):
        val = (inter / ((area + area).astype(np.float32) - inter)).astype(np.float32)
    inside = val > f32(iou)
    rows = tuple(int(sum(1 << c for c in range(2 * radius + 1) if inside[r, c])) for r in range(2 * radius + 1))
    return radius, rows


def nms_score_map(prob: torch.Tensor, protocol: str, *, conf_thresh: float, dist_thresh: Optional[int] = None, size=None, iou=None,
                  keep_top_k: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """NMS score maps of a batch (balf_nms_score_map in include/balf_hip.h): ``prob`` [B,H,W] float32 on the GPU -> (map [B,H,W]
    float32: a survivor keeps its score, everything else is +0.0; count [B] int32 survivors).  ``protocol='greedy'``: the
    reference's ``apply_nms_fast(prob[b], dist_thresh, conf_thresh)``; ``protocol='box'``: its ``box_nms(prob[b:b+1], size, iou,
    min_prob=conf_thresh, keep_top_k)`` with the footprint of :func:`box_footprint`.  Among equal scores the lower raster index
    comes first.  ``keep_top_k <= 0``: all survivors.  Nothing is read back."""
    if protocol not in NMS_MAP_PROTOCOLS:
        raise ValueError(f"protocol must be one of {sorted(NMS_MAP_PROTOCOLS)}, got {protocol!r}")
    if not isinstance(prob, torch.Tensor) or prob.dtype != torch.float32 or prob.dim() != 3:
        raise BalfHipError("prob must be a [B,H,W] float32 tensor")
    require_gpu_tensor(prob, "prob")
    if not (float(conf_thresh) > 0.0):
        raise ValueError(f"conf_thresh must be positive, got {conf_thresh}")
    radius, rows, dist = 0, None, 0
    if protocol == "greedy":
        if dist_thresh is None or int(dist_thresh) != dist_thresh or not (1 <= int(dist_thresh) <= _lib.NMS_MAP_MAX_RADIUS):
            raise ValueError(f"dist_thresh must be an integer in 1..{_lib.NMS_MAP_MAX_RADIUS}, got {dist_thresh}")
        dist = int(dist_thresh)
    else:
        if size is None or iou is None:
            raise ValueError("protocol 'box' needs size and iou")
        radius, table = box_footprint(size, iou)
        rows = (C.c_uint64 * len(table))(*table)
    b, h, w = prob.shape
    dev = prob.device
    code = NMS_MAP_PROTOCOLS[protocol]
    nbytes = C.c_size_t(0)
    check(lib().balf_nms_score_map_sizes(b, h, w, code, C.byref(nbytes)), "balf_nms_score_map_sizes")
    out = torch.empty_like(prob)
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = _workspace("nms_map", dev, nbytes.value)
    launch("balf_nms_score_map", dev, prob, b, h, w, code, float(conf_thresh), dist, rows, radius, int(keep_top_k), out, count,
           Workspace(ws))
    return out, count


def profile_begin() -> None:
    check(lib().balf_profile_begin(), "balf_profile_begin")


def profile_end():
    """-> {slot name: (total device ms, launches)} for the launches since profile_begin()."""
    l = lib()
    n = l.balf_profile_num_slots()
    ms = (C.c_float * n)()
    cnt = (C.c_int * n)()
    check(l.balf_profile_end(ms, cnt), "balf_profile_end")
    return {l.balf_profile_slot_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n) if cnt[i]}


def extract_patches(gray_u8: torch.Tensor, xy: torch.Tensor, scale: float) -> torch.Tensor:
    """uint8 gray image [H,W] + keypoints [N,2] (x, y) -> patches [N,1,32,32] fp32 in [0,1]: what
    ``K.feature.extract_patches_from_pyramid(gray/255, laf_from_center_scale_ori(kp, scale, 0), PS=32)`` returns in
    /root/reference/demo/demo_match.py:62-70 (balf_extract_patches in include/balf_hip.h)."""
    require_gpu_tensor(gray_u8, "gray_u8")
    if not xy.is_cuda:
        raise BalfHipError("xy must live on the GPU")
    if gray_u8.dtype != torch.uint8 or gray_u8.dim() != 2:
        raise BalfHipError("gray_u8 must be a [H,W] uint8 tensor")
    if xy.dim() != 2 or xy.shape[1] != 2:
        raise BalfHipError("xy must be [N,2]")
    xy = xy.contiguous().float()
    n = xy.shape[0]
    h, w = gray_u8.shape
    dev = gray_u8.device
    out = torch.empty((n, 1, 32, 32), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    nbytes = lib().balf_extract_patches_workspace_bytes(h, w, float(scale))
    ws = _workspace("patches", dev, nbytes)
    launch("balf_extract_patches", dev, gray_u8, h, w, xy, n, float(scale), out, Workspace(ws))
    return out


def rgb_to_gray_u8(rgb_u8: torch.Tensor) -> torch.Tensor:
    """uint8 RGB [...,3] on the GPU -> uint8 gray [...] with PIL's ``convert('L')`` arithmetic, which is what the
    demo's ``load_im`` feeds the patch extractor (/root/reference/demo/demo_match.py:13-19)."""
    require_gpu_tensor(rgb_u8, "rgb_u8")
    if rgb_u8.dtype != torch.uint8 or rgb_u8.shape[-1] != 3:
        raise BalfHipError("rgb_u8 must be a uint8 tensor with a last dimension of 3")
    out = torch.empty(rgb_u8.shape[:-1], dtype=torch.uint8, device=rgb_u8.device)
    if out.numel():
        launch("balf_rgb_to_gray", rgb_u8.device, rgb_u8, out.numel(), out)
    return out


def extract_patches_batch(gray_u8: torch.Tensor, xy: torch.Tensor, count, scale: float) -> torch.Tensor:
    """Batched :func:`extract_patches`: gray_u8 [B,H,W] uint8, xy [B,K,2], count [B] int32 (or None: all K valid) ->
    patches [B,K,1,32,32]; slots past an image's count are zero patches (balf_extract_patches_batch)."""
    require_gpu_tensor(gray_u8, "gray_u8")
    if gray_u8.dtype != torch.uint8 or gray_u8.dim() != 3:
        raise BalfHipError("gray_u8 must be a [B,H,W] uint8 tensor")
    if xy.dim() != 3 or xy.shape[0] != gray_u8.shape[0] or xy.shape[2] != 2 or not xy.is_cuda:
        raise BalfHipError("xy must be a [B,K,2] GPU tensor")
    xy = xy.contiguous().float()
    b, h, w = gray_u8.shape
    k = xy.shape[1]
    dev = gray_u8.device
    out = torch.empty((b, k, 1, 32, 32), dtype=torch.float32, device=dev)
    if k == 0:
        return out
    if count is not None:
        count = count.to(device=dev, dtype=torch.int32).contiguous()
    ws = _workspace("patches", dev, lib().balf_extract_patches_batch_workspace_bytes(b, h, w, float(scale)))
    launch("balf_extract_patches_batch", dev, gray_u8, b, h, w, xy, count, k, float(scale), out, Workspace(ws))
    return out


def match_smnn(desc1: torch.Tensor, desc2: torch.Tensor, th: float = 0.8) -> Tuple[torch.Tensor, torch.Tensor]:
    """``kornia.feature.match_smnn(desc1, desc2, th)`` (/root/reference/demo/demo_match.py:104-110): returns
    (dists [M,1] fp32, idxs [M,2] int64), mutual ratio-test matches sorted by the index in ``desc1``."""
    desc1, desc2 = desc1.float().contiguous(), desc2.float().contiguous()      # strided views (desc[:n]) are copied
    require_gpu_tensor(desc1, "desc1")
    require_gpu_tensor(desc2, "desc2")
    if desc1.dim() != 2 or desc2.dim() != 2 or desc1.shape[1] != 128 or desc2.shape[1] != 128:
        raise BalfHipError("descriptors must be [N,128]")
    n1, n2 = desc1.shape[0], desc2.shape[0]
    dev = desc1.device
    if n1 == 0 or n2 == 0:
        return (torch.zeros((0, 1), dtype=torch.float32, device=dev), torch.zeros((0, 2), dtype=torch.int64, device=dev))
    cap = min(n1, n2)
    idx = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((cap,), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = _workspace("match", dev, lib().balf_match_smnn_workspace_bytes(n1, n2))
    launch("balf_match_smnn", dev, desc1, n1, desc2, n2, float(th), idx, dist, count, Workspace(ws))
    m = int(count.item())
    return dist[:m].view(-1, 1), idx[:m].long()


def match_smnn_batch(desc1: torch.Tensor, n1: torch.Tensor, desc2: torch.Tensor, n2: torch.Tensor, th: float = 0.8):
    """``pairs`` independent :func:`match_smnn` problems in three launches: desc1 [P,K1,128] / desc2 [P,K2,128] with
    n1 / n2 [P] valid rows each -> (dist [P,cap] fp32, idx [P,cap,2] int32 (-1 padded), count [P] int32), cap =
    min(K1, K2); nothing is read back to the host (balf_match_smnn_batch)."""
    # strided views (full[:, :k], full[::2]) are copied: the library strides pairs by K * 128 floats
    desc1, desc2 = desc1.float().contiguous(), desc2.float().contiguous()
    require_gpu_tensor(desc1, "desc1")
    require_gpu_tensor(desc2, "desc2")
    if desc1.dim() != 3 or desc2.dim() != 3 or desc1.shape[2] != 128 or desc2.shape[2] != 128 or desc1.shape[0] != desc2.shape[0]:
        raise BalfHipError("descriptors must be [P,K,128] with the same number of pairs")
    p, k1, k2 = desc1.shape[0], desc1.shape[1], desc2.shape[1]
    dev = desc1.device
    cap = min(k1, k2)
    idx = torch.empty((p, cap, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((p, cap), dtype=torch.float32, device=dev)
    count = torch.empty((p,), dtype=torch.int32, device=dev)
    if p == 0 or cap == 0:
        return dist, idx, count.zero_()
    n1 = n1.to(device=dev, dtype=torch.int32).contiguous()
    n2 = n2.to(device=dev, dtype=torch.int32).contiguous()
    ws = _workspace("match", dev, lib().balf_match_smnn_batch_workspace_bytes(p, k1, k2))
    launch("balf_match_smnn_batch", dev, desc1, k1, n1, desc2, k2, n2, p, float(th), idx, dist, count, Workspace(ws))
    return dist, idx, count


# ---- multi-scale extraction (balf_amd/multiscale.py drives these) ----------------------------------------------------------
def pyramid_level(src: torch.Tensor, kind: int, channels: int, h_in: int, w_in: int, sigma: float, h_out: int,
                  w_out: int) -> torch.Tensor:
    """One pyramid level -> the zero-padded [B,3,Hp,Wp] fp32 batch the forward takes (balf_pyramid_level in
    include/balf_hip.h).  ``src``: uint8 [B,H,W(,3)] (kind PYR_SRC_U8), fp32 [B,H,W,3] (PYR_SRC_F32) or a level this
    function returned (PYR_SRC_LEVEL, ``channels`` 1 for a gray pyramid); ``sigma > 0`` blurs before resampling."""
    require_gpu_tensor(src, "src")
    b = src.shape[0]
    hp, wp = padded_hw(h_out, w_out)[:2]
    dev = src.device
    out = torch.empty((b, 3, hp, wp), dtype=torch.float32, device=dev)
    launch("balf_pyramid_level", dev, src, int(kind), int(channels), b, int(h_in), int(w_in), float(sigma), int(h_out), int(w_out),
           out)
    return out


def build_pyramid(images: torch.Tensor, shapes, upsampled_levels: int, sigma: float):
    """uint8 gray [B,H,W] / RGB [B,H,W,3] or float [B,H,W,3] images on the GPU -> one padded [B,3,Hp_i,Wp_i] fp32 batch per
    level of ``shapes`` (level ``upsampled_levels`` is the input itself): level U is the input as the forward's prepared
    input, the levels below it are level U resized without blur, each level above it is the one before blurred (``sigma``)
    and resized.  Stream-ordered, nothing read back."""
    require_gpu_tensor(images, "images")
    u = int(upsampled_levels)
    if images.dtype == torch.uint8:
        if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[-1] != 3):
            raise ValueError("uint8 images must be [B,H,W] (gray) or [B,H,W,3] (RGB)")
        kind, ch = _lib.PYR_SRC_U8, (1 if images.dim() == 3 else 3)
    else:
        if images.dim() != 4 or images.shape[-1] != 3 or not images.is_floating_point():
            raise ValueError("float images must be [B,H,W,3]")
        images = images.to(torch.float32).contiguous()
        kind, ch = _lib.PYR_SRC_F32, 3
    h, w = images.shape[1], images.shape[2]
    if tuple(shapes[u]) != (h, w):
        raise ValueError(f"level {u} must have the input's shape {(h, w)}, got {tuple(shapes[u])}")
    levels = [None] * len(shapes)
    levels[u] = pyramid_level(images, kind, ch, h, w, 0.0, h, w)
    for i in range(u - 1, -1, -1):
        levels[i] = pyramid_level(levels[u], _lib.PYR_SRC_LEVEL, ch, h, w, 0.0, *shapes[i])
    for i in range(u + 1, len(shapes)):
        levels[i] = pyramid_level(levels[i - 1], _lib.PYR_SRC_LEVEL, ch, *shapes[i - 1], float(sigma), *shapes[i])
    return levels


def nms_topk_budget(prob: torch.Tensor, crop_y: int, crop_x: int, h: int, w: int, border: int, nms_size: int,
                    cum_budget: int, k_max: int, taken: torch.Tensor, idx: torch.Tensor = None, score: torch.Tensor = None,
                    count: torch.Tensor = None):
    """:func:`nms_topk` with each image's K decided on the device: K_b = min(max(cum_budget - taken[b], 0), k_max, h*w), then
    ``taken[b] += count[b]`` (balf_nms_topk_budget).  ``taken`` [B] int32 on the GPU, zero before the first level.
    Returns (idx [B,k_max], score [B,k_max], count [B]); pass ``idx`` / ``score`` / ``count`` to write into given rows."""
    require_gpu_tensor(prob, "prob")
    require_gpu_tensor(taken, "taken")
    if prob.dtype != torch.float32 or prob.dim() != 3:
        raise BalfHipError("prob must be a [B,Hp,Wp] float32 tensor")
    b, hp, wp = prob.shape
    if taken.dtype != torch.int32 or taken.shape != (b,):
        raise BalfHipError("taken must be a [B] int32 tensor")
    dev = prob.device
    idx = torch.empty((b, k_max), dtype=torch.int32, device=dev) if idx is None else idx
    score = torch.empty((b, k_max), dtype=torch.float32, device=dev) if score is None else score
    count = torch.empty((b,), dtype=torch.int32, device=dev) if count is None else count
    for t, shape, dt in ((idx, (b, k_max), torch.int32), (score, (b, k_max), torch.float32), (count, (b,), torch.int32)):
        require_gpu_tensor(t, "output")
        if t.shape != shape or t.dtype != dt:
            raise BalfHipError(f"output must be {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    ws = _workspace("nms", dev, lib().balf_nms_topk_workspace_bytes(b, h, w, 1))
    launch("balf_nms_topk_budget", dev, prob, b, hp, wp, int(crop_y), int(crop_x), int(h), int(w), int(border), int(nms_size),
           int(cum_budget), int(k_max), taken, idx, score, count, Workspace(ws))
    return idx, score, count


def multiscale_merge(idx: torch.Tensor, score: torch.Tensor, count: torch.Tensor, widths, homographies, n: int,
                     order_yx: bool = False):
    """Level lists idx / score [L,B,K_max], count [L,B] -> (pts [B,n,4] float64, count [B] int32): every entry's
    (x, y, 1.0, score) mapped through its level's 3x3 homography, ordered by (score desc, level asc, index asc), the
    first n kept; (y, x, ...) with ``order_yx`` (balf_multiscale_merge)."""
    for t, name in ((idx, "idx"), (score, "score"), (count, "count")):
        require_gpu_tensor(t, name)
    if idx.dim() != 3 or score.shape != idx.shape or count.shape != idx.shape[:2]:
        raise BalfHipError("idx / score must be [L,B,K_max] and count [L,B]")
    if idx.dtype != torch.int32 or score.dtype != torch.float32 or count.dtype != torch.int32:
        raise BalfHipError("idx / count must be int32 and score float32")
    nl, b, k_max = idx.shape
    w_host = (C.c_int32 * nl)(*[int(v) for v in widths])
    hs = [float(v) for hm in homographies for v in list(np.asarray(hm, dtype=np.float64).reshape(9))]
    if len(widths) != nl or len(hs) != 9 * nl:
        raise BalfHipError(f"{nl} levels need {nl} widths and {nl} homographies")
    h_host = (C.c_double * (9 * nl))(*hs)
    dev = idx.device
    pts = torch.empty((b, n, 4), dtype=torch.float64, device=dev)
    cnt = torch.empty((b,), dtype=torch.int32, device=dev)
    launch("balf_multiscale_merge", dev, idx, score, count, nl, b, k_max, w_host, h_host, int(n), int(bool(order_yx)), pts, cnt)
    return pts, cnt


# ---- synthetic-pair validation (balf_amd/benchmark_test/evaluate.py drives this) -------------------------------------------
VAL_LEGS = {"greedy": _lib.VAL_LEG_GREEDY, "window": _lib.VAL_LEG_WINDOW}


def val_points(prob_src: torch.Tensor, prob_dst: torch.Tensor, h_dst_2_src: torch.Tensor, nms_size: int, num_points: int,
               leg: str, conf_thresh: float = 0.015):
    """The point selection of ``check_val_repeatability`` for P pairs (balf_val_points in include/balf_hip.h): score maps
    ``prob_src`` [P,Hs,Ws] / ``prob_dst`` [P,Hd,Wd] fp32 and ``h_dst_2_src`` [P,3,3] (or [P,9]) float64 on the GPU ->
    (src_pts [P,K,4] float64, dst_to_src_pts [P,K,4] float64, count [P,2] int32).  ``leg``: ``'greedy'`` (nms_fast on the
    candidates >= ``conf_thresh``) or ``'window'`` (apply_nms).  ``num_points`` beyond a map's pixels raises IndexError like
    the reference.  Nothing is read back."""
    if leg not in VAL_LEGS:
        raise ValueError(f"leg must be one of {sorted(VAL_LEGS)}, got {leg!r}")
    for t, name in ((prob_src, "prob_src"), (prob_dst, "prob_dst"), (h_dst_2_src, "h_dst_2_src")):
        require_gpu_tensor(t, name)
    for t, name in ((prob_src, "prob_src"), (prob_dst, "prob_dst")):
        if t.dtype != torch.float32 or t.dim() != 3:
            raise BalfHipError(f"{name} must be a [P,H,W] float32 tensor")
    p, hs, ws_ = prob_src.shape
    dev = prob_src.device
    if prob_dst.shape[0] != p or p == 0 or prob_dst.device != dev:
        raise BalfHipError(f"prob_src and prob_dst must hold the same number (> 0) of pairs on one device")
    hd, wd = prob_dst.shape[1:]
    if h_dst_2_src.dtype != torch.float64 or tuple(h_dst_2_src.shape) not in ((p, 3, 3), (p, 9)) or h_dst_2_src.device != dev:
        raise BalfHipError(f"h_dst_2_src must be a [{p},3,3] float64 tensor on {dev}")
    k = int(num_points)
    if k <= 0:
        raise ValueError(f"num_points must be positive, got {num_points}")
    if k > min(hs * ws_, hd * wd):
        raise IndexError(f"index {k - 1} is out of bounds for axis 0 with size {min(hs * ws_, hd * wd)}")
    nbytes = lib().balf_val_points_workspace_bytes(p, hs, ws_, hd, wd, VAL_LEGS[leg], int(nms_size), k)
    if nbytes == 0:
        raise BalfHipError(f"balf_val_points: unsupported sizes P={p}, {hs}x{ws_} / {hd}x{wd}, leg={leg}, nms_size={nms_size}, "
                           f"num_points={k}")
    src = torch.empty((p, k, 4), dtype=torch.float64, device=dev)
    dst = torch.empty((p, k, 4), dtype=torch.float64, device=dev)
    count = torch.empty((p, 2), dtype=torch.int32, device=dev)
    ws = _workspace("val_points", dev, nbytes)
    launch("balf_val_points", dev, prob_src, hs, ws_, prob_dst, hd, wd, p, h_dst_2_src, VAL_LEGS[leg], float(conf_thresh),
           int(nms_size), k, src, dst, count, Workspace(ws))
    return src, dst, count


def _check_layouts(named, dev) -> None:
    """``named``: (tensor, name, allowed shapes, dtype) tuples.  Every tensor is contiguous on the GPU ``dev``, of its dtype and of
    one of its shapes."""
    for t, name, shapes_ok, dt in named:
        require_gpu_tensor(t, name)
        if tuple(t.shape) not in shapes_ok or t.dtype != dt or t.device != dev:
            raise BalfHipError(f"{name} must be a {' or '.join(map(str, shapes_ok))} {dt} tensor on {dev}")


# ---- the resize protocol of the HSequences evaluation (benchmark_test/evaluate.py, datasets/dataset_utils.py drive these) ---
ROW_ORDERS = {"rcp": 0, "xyrs": 1}


def resize_repeatability_batch(src: torch.Tensor, ns: torch.Tensor, dst: torch.Tensor, nd: torch.Tensor, h: torch.Tensor,
                               h_inv: torch.Tensor, shapes: torch.Tensor, keep_k_points: int = 1000,
                               distance_thresh: float = 5, order: str = "rcp"):
    """``compute_resize_repeatability`` for P pairs (balf_resize_repeatability_batch in include/balf_hip.h): ``src``
    [P,Ns,C] / ``dst`` [P,Nd,C] float64 rows, ``order='rcp'``: (row, col, prob, ...) as the reference, ``'xyrs'``:
    (x, y, radius, score) as this library's detectors; ``ns`` / ``nd`` [P] int32; ``h`` / ``h_inv`` [P,3,3] (or [P,9])
    float64, ``shapes`` [P,4] int32 = (h_src, w_src, h_dst, w_dst); everything on the GPU.  Returns (rep [P,2] float64 =
    (repeatability, localization_err), counts [P,4] int32 = (N1, N2, count1, count2)); nothing is read back and no input is
    written."""
    if order not in ROW_ORDERS:
        raise ValueError(f"order must be one of {sorted(ROW_ORDERS)}, got {order!r}")
    k = int(keep_k_points)
    if k <= 0 or k > _lib.MAX_TOPK:
        raise ValueError(f"keep_k_points must be in 1..{_lib.MAX_TOPK}, got {keep_k_points}")
    if not float(distance_thresh) >= 0.0:
        raise ValueError(f"distance_thresh must be >= 0, got {distance_thresh}")
    min_c = 4 if order == "xyrs" else 3
    for t, name in ((src, "src"), (dst, "dst")):
        require_gpu_tensor(t, name)
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] < min_c:
            raise BalfHipError(f"{name} must be a [P,N,C>={min_c}] float64 tensor for order {order!r}")
    p, ns_max, nd_max = src.shape[0], src.shape[1], dst.shape[1]
    dev = src.device
    if dst.shape[0] != p or p == 0 or dst.device != dev:
        raise BalfHipError(f"src and dst must hold the same number (> 0) of pairs on one device, got {p} and {dst.shape[0]}")
    _check_layouts(((ns, "ns", ((p,),), torch.int32), (nd, "nd", ((p,),), torch.int32), (h, "h", ((p, 3, 3), (p, 9)), torch.float64),
                    (h_inv, "h_inv", ((p, 3, 3), (p, 9)), torch.float64), (shapes, "shapes", ((p, 4),), torch.int32)), dev)
    nbytes = lib().balf_resize_repeatability_batch_workspace_bytes(p, ns_max, nd_max, k)
    if nbytes == 0:
        raise BalfHipError(f"balf_resize_repeatability_batch: unsupported sizes P={p}, Ns={ns_max}, Nd={nd_max}, k={k}")
    rep = torch.empty((p, 2), dtype=torch.float64, device=dev)
    cnt = torch.empty((p, 4), dtype=torch.int32, device=dev)
    ws = _workspace("resize_repeat", dev, nbytes)
    launch("balf_resize_repeatability_batch", dev, src, ns, ns_max, src.shape[2], dst, nd, nd_max, dst.shape[2], 1,
           ROW_ORDERS[order], p, h, h_inv, shapes, k, float(distance_thresh), rep, cnt, Workspace(ws))
    return rep, cnt


def resize_crop_u8(packed: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, channels: int, target_h: int,
                   target_w: int) -> torch.Tensor:
    """``ratio_preserving_resize`` of B uint8 images of different sizes in one launch (balf_resize_crop_u8 in
    include/balf_hip.h): ``packed`` the images back to back (uint8, 1-D), ``offsets`` [B] int64 byte offsets, ``sizes`` [B,2]
    int32 (h, w), all on the GPU -> [B,target_h,target_w] (``channels`` 1) or [B,target_h,target_w,3] uint8: what
    ``pipeline.detect_batch_u8`` takes."""
    for t, name in ((packed, "packed"), (offsets, "offsets"), (sizes, "sizes")):
        require_gpu_tensor(t, name)
    b = offsets.shape[0]
    if packed.dtype != torch.uint8 or packed.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 or \
            sizes.dtype != torch.int32 or tuple(sizes.shape) != (b, 2) or b == 0:
        raise BalfHipError("packed must be a 1-D uint8 tensor, offsets [B] int64 and sizes [B,2] int32 with B > 0")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels}")
    dev = packed.device
    out = torch.empty((b, int(target_h), int(target_w)) + ((3,) if channels == 3 else ()), dtype=torch.uint8, device=dev)
    launch("balf_resize_crop_u8", dev, packed, packed.numel(), offsets, sizes, b, int(channels), int(target_h), int(target_w), out)
    return out


# ---- synthetic-homography image pairs of the validation and the training task (datasets/synthetic_pairs.py drives this) ----
def synth_pairs(packed: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, inv_h: torch.Tensor, win_src: torch.Tensor,
                win_dst: torch.Tensor, pts: torch.Tensor, pts_offsets: torch.Tensor, top_k: int, patch: int, out=None):
    """The image patches and heat maps of P synthetic-homography pairs in one call (balf_synth_pairs in include/balf_hip.h):
    ``packed`` the uint8 RGB-interleaved source images back to back (1-D), ``offsets`` [P] int64 byte offsets, ``sizes`` [P,2]
    int32 (h, w), ``inv_h`` [P,3,3] (or [P,9]) float64 -- the matrix the reference hands to ``cv2.warpPerspective`` --,
    ``win_src`` / ``win_dst`` [P,2] int32 (top row, left column), ``pts`` [N,3] float32 label rows (x, y, prob),
    ``pts_offsets`` [P+1] int32; everything on the GPU.  Returns (img_src [P,3,patch,patch], img_dst [P,3,patch,patch],
    heat_src [P,1,patch,patch], heat_dst [P,1,patch,patch] float32, dst_max [P] int32); ``out`` = such a 5-tuple to write into
    instead of allocating.  Nothing is read back: a window that leaves its image shows as ``dst_max == -1``."""
    return _synth_pairs("balf_synth_pairs", packed, offsets, sizes, inv_h, win_src, win_dst, pts, pts_offsets, top_k, patch, out, ())


def synth_train_pairs(packed: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, inv_h: torch.Tensor, win_src: torch.Tensor,
                      win_dst: torch.Tensor, pts: torch.Tensor, pts_offsets: torch.Tensor, top_k: int, patch: int,
                      params: torch.Tensor, perm: torch.Tensor, out=None):
    """:func:`synth_pairs` for the TRAINING task (balf_synth_train_pairs in include/balf_hip.h): the destination patch is the
    warp of the photometrically distorted image, ``params`` [P,5] float64 (delta_b, alpha1, sat, hue, alpha2) and ``perm`` [P]
    int32 per pair (``datasets.dataset_utils.sample_photometric``), on the GPU.  Everything else as there; a ``perm`` outside
    0..5 shows as an all-zero destination patch and ``dst_max == -1``."""
    return _synth_pairs("balf_synth_train_pairs", packed, offsets, sizes, inv_h, win_src, win_dst, pts, pts_offsets, top_k, patch,
                        out, (params, perm))


def _check_photometric(params, perm, n, dev):
    _check_layouts(((params, "params", ((n, 5),), torch.float64), (perm, "perm", ((n,),), torch.int32)), dev)


def photometric_u8(packed: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, params: torch.Tensor, perm: torch.Tensor,
                   blue_idx: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's ``bgr_distorsion`` with given parameters on B whole images in one launch (balf_photometric_u8 in
    include/balf_hip.h): ``packed`` the uint8 3-channel interleaved images back to back (1-D), ``offsets`` [B] int64, ``sizes``
    [B,2] int32 (h, w), ``params`` [B,5] float64 (delta_b, alpha1, sat, hue, alpha2), ``perm`` [B] int32, all on the GPU;
    ``blue_idx`` 0 for B, G, R pixels, 2 for R, G, B.  -> a uint8 tensor laid out as ``packed`` (``out``, which may be
    ``packed`` itself, or a new one, zeroed: an image outside ``packed`` is not written)."""
    for t, name in ((packed, "packed"), (offsets, "offsets"), (sizes, "sizes")):
        require_gpu_tensor(t, name)
    b = offsets.shape[0] if offsets.dim() == 1 else 0
    if packed.dtype != torch.uint8 or packed.dim() != 1 or offsets.dtype != torch.int64 or b == 0 or \
            sizes.dtype != torch.int32 or tuple(sizes.shape) != (b, 2):
        raise BalfHipError("packed must be a 1-D uint8 tensor, offsets [B] int64 and sizes [B,2] int32 with B > 0")
    dev = packed.device
    _check_photometric(params, perm, b, dev)
    if blue_idx not in (0, 2):
        raise ValueError(f"blue_idx must be 0 (BGR) or 2 (RGB), got {blue_idx}")
    if out is None:
        out = torch.zeros_like(packed)
    else:
        require_gpu_tensor(out, "out")
        if out.dtype != torch.uint8 or out.shape != packed.shape or out.device != dev:
            raise BalfHipError(f"out must be a uint8 tensor of {tuple(packed.shape)} on {dev}")
    launch("balf_photometric_u8", dev, packed, packed.numel(), offsets, sizes, b, params, perm, int(blue_idx), out)
    return out


def _synth_pairs(entry, packed, offsets, sizes, inv_h, win_src, win_dst, pts, pts_offsets, top_k, patch, out, photometric):
    """The body of :func:`synth_pairs` and :func:`synth_train_pairs`: ``entry`` the library's, ``photometric`` = () or
    (params, perm), which follow the workspace in the argument list."""
    for t, name in ((packed, "packed"), (offsets, "offsets"), (sizes, "sizes"), (inv_h, "inv_h"), (win_src, "win_src"),
                    (win_dst, "win_dst"), (pts, "pts"), (pts_offsets, "pts_offsets")):
        require_gpu_tensor(t, name)
    p = offsets.shape[0] if offsets.dim() == 1 else 0
    if packed.dtype != torch.uint8 or packed.dim() != 1 or offsets.dtype != torch.int64 or p == 0 or \
            sizes.dtype != torch.int32 or tuple(sizes.shape) != (p, 2):
        raise BalfHipError("packed must be a 1-D uint8 tensor, offsets [P] int64 and sizes [P,2] int32 with P > 0")
    dev = packed.device
    _check_layouts(((inv_h, "inv_h", ((p, 3, 3), (p, 9)), torch.float64), (win_src, "win_src", ((p, 2),), torch.int32),
                    (win_dst, "win_dst", ((p, 2),), torch.int32), (pts_offsets, "pts_offsets", ((p + 1,),), torch.int32)), dev)
    if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3 or pts.device != dev:
        raise BalfHipError(f"pts must be an [N,3] float32 tensor on {dev}")
    if photometric:
        _check_photometric(*photometric, p, dev)
    top_k, patch = int(top_k), int(patch)
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0 (0 keeps every row), got {top_k}")
    if patch <= 0:
        raise ValueError(f"patch must be positive, got {patch}")
    nbytes = lib().balf_synth_pairs_workspace_bytes(p, patch)
    if nbytes == 0:
        raise BalfHipError(f"{entry}: unsupported sizes P={p}, patch={patch}")
    shapes = ((p, 3, patch, patch), (p, 3, patch, patch), (p, 1, patch, patch), (p, 1, patch, patch), (p,))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32 if len(s) == 1 else torch.float32, device=dev) for s in shapes)
    else:
        if len(out) != 5:
            raise BalfHipError("out must be (img_src, img_dst, heat_src, heat_dst, dst_max)")
        for t, s in zip(out, shapes):
            require_gpu_tensor(t, "out")
            if tuple(t.shape) != s or t.dtype != (torch.int32 if len(s) == 1 else torch.float32) or t.device != dev:
                raise BalfHipError(f"out tensors must be {shapes} (float32, dst_max int32) on {dev}")
    ws = _workspace("synth_pairs", dev, nbytes)
    launch(entry, dev, packed, packed.numel(), offsets, sizes, p, inv_h, win_src, win_dst,
           pts if pts.shape[0] else None, pts.shape[0], pts_offsets, top_k, patch, *out, Workspace(ws), *photometric)
    return tuple(out)


def _check_devices(named, anchor, dev) -> None:
    """Every tensor of ``named`` ((tensor or None, name, ...) tuples) is on a GPU, and on ``dev``, the device of ``anchor``."""
    for t, name, *_ in named:
        if t is not None:
            require_gpu_tensor(t, name)
            if t.device != dev:
                raise BalfHipError(f"{name} is on {t.device}, {anchor} on {dev}")


def _check_metadata(named, aligned=(), strict_saved=False) -> None:
    """``named``: (tensor or None, name, shape or None) triples.  Every tensor is float32, of its shape and contiguous; those
    named in ``aligned`` (True: all) start on a 16-byte boundary of their storage.  ``saved`` is the opaque uint8 block of a
    training unit: contiguous (``strict_saved``: and uint8, in one message); _saved_block checks the rest."""
    for t, name, shape in named:
        if t is None:
            continue
        if name == "saved":
            if strict_saved and (t.dtype != torch.uint8 or not t.is_contiguous()):
                raise BalfHipError("saved must be a contiguous uint8 tensor")
            if not t.is_contiguous():
                raise BalfHipError("saved must be contiguous")
            continue
        if t.dtype != torch.float32:
            raise BalfHipError(f"{name} must be float32, got {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise BalfHipError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        if not t.is_contiguous():
            raise BalfHipError(f"{name} must be contiguous")
        if (aligned is True or name in aligned) and t.storage_offset() * t.element_size() % 16:
            raise BalfHipError(f"{name} must start on a 16-byte boundary of its storage")


def _check_tensors(named, anchor, aligned=(), strict_saved=False) -> None:
    """The checks of a training unit's tensors, the anchor (whose device the others must share) first in ``named``: all of
    _check_metadata, then the devices, so that a wrong call is refused before any device is touched."""
    _check_metadata(named, aligned, strict_saved)
    _check_devices(named, anchor, named[0][0].device)


def _saved_block(saved, need: int, dev, align16: bool, made_by: Optional[str] = None) -> torch.Tensor:
    """The ``saved`` block of a training unit.  Forward (``made_by`` None): allocated when None, else a uint8 tensor of at least
    ``need`` bytes (``align16``: that starts on 16 bytes).  Backward: the same demands on the block that forward ``made_by``
    returned."""
    if saved is None and made_by is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if saved is None or saved.dtype != torch.uint8 or saved.numel() < need or (align16 and saved.data_ptr() % 16):
        if made_by is not None:
            raise BalfHipError(f"saved must be the uint8 block that {made_by} returned for this shape")
        raise BalfHipError(f"saved must be a {'16-byte aligned ' if align16 else ''}uint8 tensor of at least {need} bytes")
    return saved


def _stage4_input_checks(what: str, workspace, b: int, hp: int, wp: int, conv0_w, conv0_b, outs) -> None:
    """The checks of rcab_inputs and gmlp_input: ``outs`` are (tensor, name) pairs of [b,hp/8,wp/8,256] outputs."""
    if hp <= 0 or wp <= 0 or hp % 64 or wp % 64 or b < 1:
        raise BalfHipError(f"{what}: b >= 1 and hp, wp multiples of 64, got {(b, hp, wp)}")
    shape = (b, hp // 8, wp // 8, 256)
    named = ((conv0_w, "conv0_w", (256, 128)), (conv0_b, "conv0_b", (256,))) + tuple((t, k, shape) for t, k in outs)
    _check_metadata(named)
    if workspace.dtype != torch.uint8:
        raise BalfHipError("workspace must be the uint8 workspace of the forward")
    _check_devices(((workspace, "workspace"),) + named, "the workspace", workspace.device)


class DetectorLoss(NamedTuple):
    loss: torch.Tensor                        # [] float32
    per_image: Optional[torch.Tensor]         # [B] float32
    labels: Optional[torch.Tensor]            # [B,Hc,Wc] int32
    dlogits: Optional[torch.Tensor]           # [B,65,Hc,Wc] float32


def detector_loss(logits: torch.Tensor, keypoint_map: torch.Tensor, valid_mask=None, noise=None, want_per_image: bool = False,
                  want_labels: bool = False, want_grad: bool = False) -> DetectorLoss:
    """The reference's detector_loss (/root/reference/balf/loss/loss_function.py:7-26) for grid_size 8 and, with
    ``want_grad``, its gradient with respect to the logits: balf_detector_loss in include/balf_hip.h.  ``logits``
    [B,65,Hc,Wc], ``keypoint_map`` and ``valid_mask`` (None = all ones) [B,1,8Hc,8Wc], ``noise`` (None = no tie-break noise)
    [B,65,Hc,Wc], all float32 and contiguous on one GPU.  Fields that were not requested are None."""
    # shapes, dtypes and contiguity from the tensors' metadata first: a wrong call is refused before any device is touched
    if logits.dim() != 4 or logits.shape[1] != 65:
        raise BalfHipError(f"logits must be [B,65,Hc,Wc] (the 65-channel head, cell size 8), got {tuple(logits.shape)}")
    b, _, hc, wc = logits.shape
    if not 1 <= b <= 65535 or hc < 1 or wc < 1 or hc * wc > 1 << 24:
        raise BalfHipError(f"detector_loss: 1 <= B <= 65535 and 1 <= Hc * Wc <= 2^24, got {tuple(logits.shape)}")
    for t, name, shape in ((logits, "logits", None), (keypoint_map, "keypoint_map", (b, 1, 8 * hc, 8 * wc)),
                           (valid_mask, "valid_mask", (b, 1, 8 * hc, 8 * wc)), (noise, "noise", (b, 65, hc, wc))):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise BalfHipError(f"{name} must be float32, got {t.dtype}")
        if shape is not None and tuple(t.shape) != shape:
            raise BalfHipError(f"{name} must be {list(shape)} for logits {list(logits.shape)}, got {list(t.shape)}")
        if not t.is_contiguous():
            raise BalfHipError(f"{name} must be contiguous")
    dev = logits.device
    _check_devices(((logits, "logits"), (keypoint_map, "keypoint_map"), (valid_mask, "valid_mask"), (noise, "noise")), "logits",
                   dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    per_image = torch.empty((b,), dtype=torch.float32, device=dev) if want_per_image else None
    labels = torch.empty((b, hc, wc), dtype=torch.int32, device=dev) if want_labels else None
    dlogits = torch.empty_like(logits) if want_grad else None
    ws = _workspace("detector_loss", dev, lib().balf_detector_loss_workspace_bytes(b, hc, wc))
    launch("balf_detector_loss", dev, logits, keypoint_map, valid_mask, noise, b, hc, wc, loss, per_image, labels, dlogits,
           Workspace(ws))
    return DetectorLoss(loss, per_image, labels, dlogits)


class HeadTrainForward(NamedTuple):
    logits: torch.Tensor                      # [B,65,Hc,Wc] float32
    prob: Optional[torch.Tensor]              # [B,8Hc,8Wc] float32
    saved: torch.Tensor                       # opaque uint8 block for head_train_backward


class HeadTrainBackward(NamedTuple):
    dw2: torch.Tensor                         # [256,256]
    db2: torch.Tensor                         # [256]
    dwd: torch.Tensor                         # [65,256]
    dbd: torch.Tensor                         # [65]
    dgamma: torch.Tensor                      # [65]
    dbeta: torch.Tensor                       # [65]
    dx2: Optional[torch.Tensor]               # [B,Hc,Wc,256]


_HEAD_PARAM_SHAPES = {"w2": (256, 256), "b2": (256,), "wd": (65, 256), "bd": (65,), "gamma": (65,), "beta": (65,),
                      "running_mean": (65,), "running_var": (65,), "stats": (2, 65)}


def _head_train_checks(x2, named):
    """``named``: (tensor or None, name, shape) triples, x2 first (_check_tensors).  -> (B, Hc, Wc)."""
    if x2.dim() != 4 or x2.shape[3] != 256:
        raise BalfHipError(f"x2 must be [B,Hc,Wc,256] (the stage-4 activation, NHWC), got {tuple(x2.shape)}")
    b, hc, wc, _ = x2.shape
    if not 1 <= b <= 65535 or hc < 1 or wc < 1 or not 2 <= b * hc * wc <= 1 << 24:
        raise BalfHipError(f"head_train: 1 <= B <= 65535 and 2 <= B * Hc * Wc <= 2^24, got {tuple(x2.shape)}")
    _check_tensors(named, "x2")
    return b, hc, wc


def head_train_forward(x2: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, wd: torch.Tensor, bd: torch.Tensor,
                       gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, stats=None, want_prob=True,
                       running_mean=None, running_var=None, momentum: float = 0.1, saved=None) -> HeadTrainForward:
    """down4.conv2 -> ReLU -> detector_head.dense -> BatchNorm2d on ``x2`` [B,Hc,Wc,256] (balf_head_train_forward in
    include/balf_hip.h).  ``stats`` None: batch statistics (training mode), and ``running_mean`` / ``running_var`` [65], when
    given, are updated in place by the kernel; ``stats`` [2,65] (mean, variance): normalise with them (eval mode).  All tensors
    float32 and contiguous on one GPU.  ``want_prob`` may be a contiguous float32 [B,8Hc,8Wc] tensor to write into.  ``saved``: a
    uint8 block to reuse (at least balf_head_train_saved_bytes), else allocated."""
    s = _HEAD_PARAM_SHAPES
    prob = want_prob if isinstance(want_prob, torch.Tensor) else None
    prob_shape = (x2.shape[0], 8 * x2.shape[1], 8 * x2.shape[2]) if x2.dim() == 4 else None
    b, hc, wc = _head_train_checks(x2, ((x2, "x2", None), (prob, "prob", prob_shape), (w2, "w2", s["w2"]), (b2, "b2", s["b2"]),
                                        (wd, "wd", s["wd"]),
                                        (bd, "bd", s["bd"]), (gamma, "gamma", s["gamma"]), (beta, "beta", s["beta"]),
                                        (stats, "stats", s["stats"]), (running_mean, "running_mean", s["running_mean"]),
                                        (running_var, "running_var", s["running_var"]), (saved, "saved", None)))
    dev, n = x2.device, b * hc * wc
    l = lib()
    saved = _saved_block(saved, l.balf_head_train_saved_bytes(n), dev, False)
    logits = torch.empty((b, 65, hc, wc), dtype=torch.float32, device=dev)
    if prob is None and want_prob:
        prob = torch.empty((b, 8 * hc, 8 * wc), dtype=torch.float32, device=dev)
    ws = _workspace("head_train", dev, l.balf_head_train_workspace_bytes(n))
    launch("balf_head_train_forward", dev, x2, w2, b2, wd, bd, gamma, beta, b, hc, wc, float(eps), 0 if stats is None else 1, stats,
           logits, prob, running_mean, running_var, float(momentum), saved, Workspace(ws))
    return HeadTrainForward(logits, prob, saved)


def head_train_backward(dlogits: torch.Tensor, x2: torch.Tensor, w2: torch.Tensor, wd: torch.Tensor, gamma: torch.Tensor,
                        saved: torch.Tensor, want_dx2=False) -> HeadTrainBackward:
    """The backward of ``head_train_forward`` in training mode (balf_head_train_backward): ``dlogits`` [B,65,Hc,Wc] and the
    ``saved`` block of that forward -> the six parameter gradients and, with ``want_dx2``, the gradient of ``x2``
    (``want_dx2`` may be a contiguous float32 tensor of x2's shape to write into)."""
    s = _HEAD_PARAM_SHAPES
    dx2 = want_dx2 if isinstance(want_dx2, torch.Tensor) else None
    shape = (x2.shape[0], 65, x2.shape[1], x2.shape[2]) if x2.dim() == 4 else None
    b, hc, wc = _head_train_checks(x2, ((x2, "x2", None), (dlogits, "dlogits", shape), (w2, "w2", s["w2"]), (wd, "wd", s["wd"]),
                                        (gamma, "gamma", s["gamma"]), (saved, "saved", None), (dx2, "dx2", tuple(x2.shape))))
    dev, n = x2.device, b * hc * wc
    l = lib()
    _saved_block(saved, l.balf_head_train_saved_bytes(n), dev, False, "head_train_forward")
    if dx2 is None and want_dx2:
        dx2 = torch.empty_like(x2)
    out = [torch.empty(s[k], dtype=torch.float32, device=dev) for k in ("w2", "b2", "wd", "bd", "gamma", "beta")]
    ws = _workspace("head_train", dev, l.balf_head_train_workspace_bytes(n))
    launch("balf_head_train_backward", dev, dlogits, x2, w2, wd, gamma, saved, b, hc, wc, *out, dx2, Workspace(ws))
    return HeadTrainBackward(*out, dx2)


RCAB_PARAMS = ("ln_g", "ln_b", "wc1", "bc1", "wc2", "bc2", "ws0", "bs0", "ws2", "bs2")
_RCAB_BACKWARD_READS = ("ln_g", "wc1", "wc2", "ws0", "ws2")
TRAIN_WIDTHS = {256: 4, 128: 3}           # channels of the RCAB and the gated-MLP layer in training form -> the Down stage


def _train_width(channels: int, what: str) -> int:
    if channels not in TRAIN_WIDTHS:
        raise BalfHipError(f"{what}: channels must be one of {sorted(TRAIN_WIDTHS)}, got {channels!r}")
    return channels


def _rcab_shapes(c: int) -> dict:
    return {"ln_g": (c,), "ln_b": (c,), "wc1": (c, c), "bc1": (c,), "wc2": (c, c), "bc2": (c,), "ws0": (c // 4, c), "bs0": (c // 4,),
            "ws2": (c, c // 4), "bs2": (c,)}


_RCAB_SHAPES = {c: _rcab_shapes(c) for c in TRAIN_WIDTHS}       # made once: every training step asks, several times
_RCAB_PARAM_SHAPES = _RCAB_SHAPES[256]                          # stage 4's, by the name the guard tests read


def rcab_param_shapes(channels: int = 256) -> dict:
    """The shapes of the ten ``RCAB_PARAMS`` of the channel-attention block at ``channels`` (256: stage 4's, 128: stage 3's): one
    dict per width, not to be modified."""
    return _RCAB_SHAPES[_train_width(channels, "rcab_param_shapes")]


def train_unit_sizes(unit: int, channels: int, b: int, h: int, w: int) -> Tuple[int, int]:
    """(workspace bytes, saved bytes) of a training unit (_lib.UNIT_RCAB / UNIT_GMLP / UNIT_POOL) at ``channels`` on ``b`` maps of
    ``h x w``, the map the unit receives: balf_train_unit_sizes in include/balf_hip.h."""
    ws, sv = C.c_size_t(0), C.c_size_t(0)
    _lib.check(lib().balf_train_unit_sizes(unit, channels, b, h, w, C.byref(ws), C.byref(sv)), "balf_train_unit_sizes")
    return ws.value, sv.value


class RcabTrainForward(NamedTuple):
    x2: torch.Tensor                          # [B,Hc,Wc,channels] float32: the block's output (stage 4: the input of down4.conv2)
    saved: torch.Tensor                       # opaque uint8 block for rcab_train_backward


class RcabTrainBackward(NamedTuple):
    dln_g: torch.Tensor                       # the ten gradients, in RCAB_PARAMS order
    dln_b: torch.Tensor
    dwc1: torch.Tensor
    dbc1: torch.Tensor
    dwc2: torch.Tensor
    dbc2: torch.Tensor
    dws0: torch.Tensor
    dbs0: torch.Tensor
    dws2: torch.Tensor
    dbs2: torch.Tensor
    dy: Optional[torch.Tensor]                # [B,Hc,Wc,channels]


def _rcab_train_checks(y, named, aligned=(), channels=256):
    """``named``: (tensor or None, name, shape) triples, y first; ``aligned``: the names whose storage must start on 16 bytes (the
    LayerNorm kernels move four channels at a time) (_check_tensors).  -> (B, Hc, Wc)."""
    if y.dim() != 4 or y.shape[3] != channels:
        raise BalfHipError(f"y must be [B,Hc,Wc,{channels}] (the input of stage {TRAIN_WIDTHS[channels]}'s RCAB, NHWC), "
                           f"got {tuple(y.shape)}")
    b, hc, wc, _ = y.shape
    if not 1 <= b <= 65535 or hc < 1 or wc < 1 or not 2 <= b * hc * wc <= 1 << 24:
        raise BalfHipError(f"rcab_train: 1 <= B <= 65535 and 2 <= B * Hc * Wc <= 2^24, got {tuple(y.shape)}")
    _check_tensors(named, "y", aligned)
    return b, hc, wc


def rcab_train_forward(y: torch.Tensor, r: torch.Tensor, params, saved=None, *, channels: int = 256) -> RcabTrainForward:
    """A Down stage's channel-attention block on ``y`` [B,Hc,Wc,channels] with ``r`` = y + the long shortcut (at stage 4,
    ``rcab_inputs`` / ``MLP_MA_DECODER.encode(level="rcab")`` give both): LayerNorm, conv1, LeakyReLU, conv2, the squeeze-excite scale
    of ``channels // 4`` units, ``x2 = t * s + r`` (balf_rcab_train_forward_c in include/balf_hip.h).  ``params``: the ten tensors in
    ``RCAB_PARAMS`` order (``rcab_param_shapes(channels)``), float32 and contiguous on y's GPU.  ``saved``: a uint8 block to reuse
    (at least the saved bytes of ``train_unit_sizes``), else allocated.  ``channels``: the block's width, a key of ``TRAIN_WIDTHS``;
    it is stated, never taken from ``y``."""
    shapes = rcab_param_shapes(channels)
    params = tuple(params)
    if len(params) != len(RCAB_PARAMS):
        raise BalfHipError(f"rcab_train_forward takes the ten parameters {RCAB_PARAMS}, got {len(params)}")
    named = ((y, "y", None), (r, "r", tuple(y.shape))) + tuple((t, k, shapes[k]) for t, k in zip(params, RCAB_PARAMS))
    b, hc, wc = _rcab_train_checks(y, named + ((saved, "saved", None),), aligned=("y", "r", "ln_g", "ln_b"), channels=channels)
    dev = y.device
    ws_bytes, saved_bytes = train_unit_sizes(_lib.UNIT_RCAB, channels, b, hc, wc)
    saved = _saved_block(saved, saved_bytes, dev, True)
    x2 = torch.empty_like(y)
    ws = _workspace("rcab_train", dev, ws_bytes)
    launch("balf_rcab_train_forward_c", dev, y, r, *params, b, hc, wc, channels, x2, saved, Workspace(ws))
    return RcabTrainForward(x2, saved)


def rcab_train_backward(dx2: torch.Tensor, y: torch.Tensor, ln_g: torch.Tensor, wc1: torch.Tensor, wc2: torch.Tensor,
                        ws0: torch.Tensor, ws2: torch.Tensor, saved: torch.Tensor, want_dy=False, *,
                        channels: int = 256) -> RcabTrainBackward:
    """The backward of ``rcab_train_forward`` (balf_rcab_train_backward_c): ``dx2`` [B,Hc,Wc,channels] (at stage 4,
    ``head_train_backward`` writes it) and the ``saved`` block of that forward -> the ten parameter gradients and, with ``want_dy``, the gradient at the block's
    input (``want_dy`` may be a contiguous float32 tensor of y's shape to write into).  ``channels`` as in the forward."""
    s = rcab_param_shapes(channels)
    dy = want_dy if isinstance(want_dy, torch.Tensor) else None
    shape = tuple(y.shape)
    named = ((y, "y", None), (dx2, "dx2", shape), (ln_g, "ln_g", s["ln_g"]), (wc1, "wc1", s["wc1"]), (wc2, "wc2", s["wc2"]),
             (ws0, "ws0", s["ws0"]), (ws2, "ws2", s["ws2"]), (saved, "saved", None), (dy, "dy", shape))
    b, hc, wc = _rcab_train_checks(y, named, aligned=("y", "ln_g"), channels=channels)
    dev = y.device
    ws_bytes, saved_bytes = train_unit_sizes(_lib.UNIT_RCAB, channels, b, hc, wc)
    _saved_block(saved, saved_bytes, dev, True, "rcab_train_forward")
    if dy is None and want_dy:
        dy = torch.empty_like(y)
    out = [torch.empty(s[k], dtype=torch.float32, device=dev) for k in RCAB_PARAMS]
    ws = _workspace("rcab_train", dev, ws_bytes)
    launch("balf_rcab_train_backward_c", dev, dx2, y, ln_g, wc1, wc2, ws0, ws2, saved, b, hc, wc, channels, *out, dy, Workspace(ws))
    return RcabTrainBackward(*out, dy)


def rcab_inputs(precision: int, workspace: torch.Tensor, b: int, hp: int, wp: int, conv0_w: torch.Tensor, conv0_b: torch.Tensor,
                y: torch.Tensor, r: torch.Tensor) -> None:
    """After a forward of ``b`` padded ``hp x wp`` images whose workspace is ``workspace`` (balf_forward_rcab_inputs): write the
    RCAB's input into ``y`` and y + the long shortcut into ``r``, both [b,hp/8,wp/8,256] float32 and contiguous on the
    workspace's GPU; ``conv0_w`` [256,128], ``conv0_b`` [256] are ``down4.conv.0``.  ``precision``: _lib.PREC_FP32 / PREC_FP16,
    the kernels that forward ran on."""
    _stage4_input_checks("rcab_inputs", workspace, b, hp, wp, conv0_w, conv0_b, ((y, "y"), (r, "r")))
    launch("balf_forward_rcab_inputs", workspace.device, precision, Workspace(workspace), b, hp, wp, conv0_w, conv0_b, y, r)


_GMLP_BRANCH = ("norm.weight", "norm.bias", "dense1.weight", "dense1.bias", "{u}.norm.weight", "{u}.norm.bias", "{u}.dense.weight",
                "{u}.dense.bias", "dense2.weight", "dense2.bias")
# the 26 parameters of a Down stage's residual_split_head_multi_axis_gmlp_layer under their state-dict names, in the order of
# include/balf_hip.h
GMLP_PARAMS = (("norm.weight", "norm.bias", "dense1.weight", "dense1.bias")
               + tuple(f"{layer}.{n.format(u=unit)}" for layer, unit in (("grid_gmlp_layer", "grid_gating_unit"),
                                                                         ("block_gmlp_layer", "block_gating_unit"))
                       for n in _GMLP_BRANCH)
               + ("dense2.weight", "dense2.bias"))


def _gmlp_shapes(c: int) -> dict:
    branch = ((c,), (c,), (2 * c, c), (2 * c,), (c,), (c,), (64, 64), (64,), (c, c), (c,))
    return dict(zip(GMLP_PARAMS, ((c,), (c,), (2 * c, c), (2 * c,)) + 2 * branch + ((c, 2 * c), (c,))))


_GMLP_SHAPES = {c: _gmlp_shapes(c) for c in TRAIN_WIDTHS}       # made once, as _RCAB_SHAPES
_GMLP_PARAM_SHAPES = _GMLP_SHAPES[256]                          # stage 4's, by the name the tests read


def gmlp_param_shapes(channels: int = 256) -> dict:
    """The shapes of the 26 ``GMLP_PARAMS`` of the gated-MLP layer at ``channels`` (256: stage 4's, 128: stage 3's); the token
    matrices stay [64,64].  One dict per width, not to be modified."""
    return _GMLP_SHAPES[_train_width(channels, "gmlp_param_shapes")]


class GmlpTrainForward(NamedTuple):
    y: torch.Tensor                           # [B,Hc,Wc,channels] float32: the input of the stage's RCAB
    saved: torch.Tensor                       # opaque uint8 block for gmlp_train_backward


class GmlpTrainBackward(NamedTuple):
    grads: Tuple[torch.Tensor, ...]           # the 26 gradients, in GMLP_PARAMS order
    dx0: Optional[torch.Tensor]               # [B,Hc,Wc,channels]


def _gmlp_train_checks(x0, params, others, channels=256):
    """``others``: (tensor or None, name, shape) triples behind x0 and the parameters.  Every tensor but ``saved`` is float32,
    contiguous and starts on a 16-byte boundary of its storage (_check_tensors).  -> (B, Hc, Wc, params)."""
    shapes = gmlp_param_shapes(channels)
    if x0.dim() != 4 or x0.shape[3] != channels:
        raise BalfHipError(f"x0 must be [B,Hc,Wc,{channels}] (the input of stage {TRAIN_WIDTHS[channels]}'s gMLP layer, NHWC), "
                           f"got {tuple(x0.shape)}")
    b, hc, wc, _ = x0.shape
    if not 1 <= b <= 65535 or hc < 1 or wc < 1 or hc % 8 or wc % 8 or b * hc * wc > 1 << 24:
        raise BalfHipError(f"gmlp_train: 1 <= B <= 65535, Hc and Wc multiples of 8 and B * Hc * Wc <= 2^24, got {tuple(x0.shape)}")
    params = tuple(params)
    if len(params) != len(GMLP_PARAMS):
        raise BalfHipError(f"gmlp_train takes the {len(GMLP_PARAMS)} parameters of ops.GMLP_PARAMS, got {len(params)}")
    named = ((x0, "x0", None),) + tuple((t, k, shapes[k]) for t, k in zip(params, GMLP_PARAMS)) + tuple(others)
    _check_tensors(named, "x0", aligned=True, strict_saved=True)
    return b, hc, wc, params


def _pointer_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def gmlp_train_forward(x0: torch.Tensor, params, saved=None, *, channels: int = 256) -> GmlpTrainForward:
    """A Down stage's multi-axis gated-MLP layer on ``x0`` [B,Hc,Wc,channels] (at stage 4,
    ``MLP_MA_DECODER.encode(level="gmlp")`` gives it): balf_gmlp_train_forward_c in include/balf_hip.h.  ``params``: the 26 tensors in
    ``GMLP_PARAMS`` order (``gmlp_param_shapes(channels)``), float32 and contiguous on x0's GPU.  ``saved``: a uint8 block to reuse
    (at least the saved bytes of ``train_unit_sizes``), else allocated.  ``channels``: the layer's width, a key of ``TRAIN_WIDTHS``;
    stated, never taken from ``x0``."""
    b, hc, wc, params = _gmlp_train_checks(x0, params, ((saved, "saved", None),), channels)
    dev = x0.device
    ws_bytes, saved_bytes = train_unit_sizes(_lib.UNIT_GMLP, channels, b, hc, wc)
    saved = _saved_block(saved, saved_bytes, dev, True)
    y = torch.empty_like(x0)
    ws = _workspace("gmlp_train", dev, ws_bytes)
    launch("balf_gmlp_train_forward_c", dev, x0, _pointer_array(params), b, hc, wc, channels, y, saved, Workspace(ws))
    return GmlpTrainForward(y, saved)


def gmlp_train_backward(dy: torch.Tensor, x0: torch.Tensor, params, saved: torch.Tensor, want_dx0=False, *,
                        channels: int = 256) -> GmlpTrainBackward:
    """The backward of ``gmlp_train_forward`` (balf_gmlp_train_backward_c): ``dy`` [B,Hc,Wc,channels] (``rcab_train_backward`` writes it)
    and the ``saved`` block of that forward -> the 26 parameter gradients and, with ``want_dx0``, the gradient at the layer's input
    through the layer (``want_dx0`` may be a contiguous float32 tensor of x0's shape to write into).  ``channels`` as in the
    forward."""
    dx0 = want_dx0 if isinstance(want_dx0, torch.Tensor) else None
    shape = tuple(x0.shape)
    b, hc, wc, params = _gmlp_train_checks(x0, params, ((dy, "dy", shape), (saved, "saved", None), (dx0, "dx0", shape)), channels)
    dev = x0.device
    ws_bytes, saved_bytes = train_unit_sizes(_lib.UNIT_GMLP, channels, b, hc, wc)
    _saved_block(saved, saved_bytes, dev, True, "gmlp_train_forward")
    if dx0 is None and want_dx0:
        dx0 = torch.empty_like(x0)
    shapes = gmlp_param_shapes(channels)
    out = tuple(torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in GMLP_PARAMS)
    ws = _workspace("gmlp_train", dev, ws_bytes)
    launch("balf_gmlp_train_backward_c", dev, dy, x0, _pointer_array(params), saved, b, hc, wc, channels, _pointer_array(out), dx0,
           Workspace(ws))
    return GmlpTrainBackward(out, dx0)


def gmlp_input(precision: int, workspace: torch.Tensor, b: int, hp: int, wp: int, conv0_w: torch.Tensor, conv0_b: torch.Tensor,
               x0: torch.Tensor) -> None:
    """After a forward of ``b`` padded ``hp x wp`` images whose workspace is ``workspace`` (balf_forward_gmlp_input): write the
    input of stage 4's gMLP layer into ``x0`` [b,hp/8,wp/8,256], float32 and contiguous on the workspace's GPU; ``conv0_w``
    [256,128], ``conv0_b`` [256] are ``down4.conv.0``.  ``precision``: _lib.PREC_FP32 / PREC_FP16, the kernels that forward ran on."""
    _stage4_input_checks("gmlp_input", workspace, b, hp, wp, conv0_w, conv0_b, ((x0, "x0"),))
    dev = workspace.device
    scratch = None
    if precision == _lib.PREC_FP16:
        scratch = _workspace("gmlp_input", dev, x0.numel() // 2 * 4)
    launch("balf_forward_gmlp_input", dev, precision, Workspace(workspace), b, hp, wp, conv0_w, conv0_b, x0, scratch)


class PoolTrainForward(NamedTuple):
    out: torch.Tensor                         # [B,H/2,W/2,C] float32
    which: torch.Tensor                       # [B,H/2,W/2,C] uint8: the raster position 0..3 of the chosen element in its window


def _pool_train_checks(anchor, name, named, scale):
    """``anchor`` [B,h,w,C] is ``x`` (the input map, ``scale`` 1) or ``g`` (the pooled map, ``scale`` 2).  -> (B, h, w, C)."""
    if anchor.dim() != 4 or anchor.shape[3] % 4 or not 4 <= anchor.shape[3] <= 256:
        raise BalfHipError(f"{name} must be [B,H,W,C] (NHWC) with C a multiple of 4 up to 256, got {tuple(anchor.shape)}")
    b, h, w, c = anchor.shape
    if not 1 <= b <= 65535 or h < 1 or w < 1:
        raise BalfHipError(f"pool_train: 1 <= B <= 65535 and H, W >= 1, got {tuple(anchor.shape)}")
    if scale == 1 and (h % 2 or w % 2):
        raise BalfHipError(f"pool_train: H and W of the input map must be even, got {tuple(anchor.shape)}")
    if b * h * w * scale * scale > 1 << 24:
        raise BalfHipError(f"pool_train: B * H * W <= 2^24 on the input map, got {tuple(anchor.shape)}")
    _check_metadata(tuple(t for t in named if t[1] != "which"), aligned=True)
    for t, k, shape in named:
        if k == "which" and (t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                             or t.storage_offset() % 16):
            raise BalfHipError(f"which must be the contiguous uint8 {list(shape)} tensor that pool_train_forward returned")
    _check_devices(tuple(t[:2] for t in named), name, anchor.device)
    return b, h, w, c


def pool_train_forward(x: torch.Tensor) -> PoolTrainForward:
    """The 2 x 2 max-pool that ends a Down stage on ``x`` [B,H,W,C] float32 NHWC, H and W even, C a multiple of 4 up to 256
    (balf_pool_train_forward in include/balf_hip.h): torch's CPU ``max_pool2d`` rule, and ``which`` for the backward."""
    b, h, w, c = _pool_train_checks(x, "x", ((x, "x", None),), 1)
    dev = x.device
    out = torch.empty((b, h // 2, w // 2, c), dtype=torch.float32, device=dev)
    which = torch.empty(train_unit_sizes(_lib.UNIT_POOL, c, b, h, w)[1], dtype=torch.uint8, device=dev).view(out.shape)
    launch("balf_pool_train_forward", dev, x, b, h, w, c, out, which)
    return PoolTrainForward(out, which)


def pool_train_backward(g: torch.Tensor, which: torch.Tensor) -> torch.Tensor:
    """The backward of ``pool_train_forward`` (balf_pool_train_backward): ``g`` [B,H/2,W/2,C] and that forward's ``which`` ->
    ``dx`` [B,H,W,C], every element written: g at the recorded position, +0 at the other three."""
    b, ho, wo, c = _pool_train_checks(g, "g", ((g, "g", None), (which, "which", tuple(g.shape))), 2)
    dev = g.device
    dx = torch.empty((b, 2 * ho, 2 * wo, c), dtype=torch.float32, device=dev)
    launch("balf_pool_train_backward", dev, g, which, b, 2 * ho, 2 * wo, c, dx)
    return dx


LINRELU_PARAMS = ("weight", "bias")       # of the Linear c_in -> 2 c_in in front of a ReLU (down4.conv.0 at c_in = 128)
_LINRELU_WIDTHS = (32, 64, 128)


class LinreluTrainForward(NamedTuple):
    y: torch.Tensor                           # [..., 2 c_in] float32: relu(x w^T + b)


class LinreluTrainBackward(NamedTuple):
    dweight: torch.Tensor                     # [2 c_in, c_in]
    dbias: torch.Tensor                       # [2 c_in]
    dx: Optional[torch.Tensor]                # as x


def _linrelu_train_checks(x, weight, others):
    """``others``: (tensor or None, name, shape) triples behind x and weight.  Every tensor is float32, contiguous and starts on a
    16-byte boundary of its storage (_check_tensors).  -> (N, c_in)."""
    if x.dim() < 2 or x.shape[-1] not in _LINRELU_WIDTHS:
        raise BalfHipError(f"x must be [..., c_in] with c_in one of {_LINRELU_WIDTHS} (pixels by channels, NHWC), got {tuple(x.shape)}")
    c_in = x.shape[-1]
    n = x.numel() // c_in
    if not 1 <= n <= 1 << 24:
        raise BalfHipError(f"linrelu_train: 1 <= N <= 2^24 pixels, got {tuple(x.shape)}")
    _check_tensors(((x, "x", None), (weight, "weight", (2 * c_in, c_in))) + tuple(others), "x", aligned=True)
    return n, c_in


def linrelu_train_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> LinreluTrainForward:
    """``relu(x weight^T + bias)`` per pixel (balf_linrelu_train_forward in include/balf_hip.h): ``x`` [..., c_in] with c_in of 32, 64
    or 128, ``weight`` [2 c_in, c_in], ``bias`` [2 c_in], float32 and contiguous on one GPU.  At c_in = 128 with ``down4.conv.0`` and
    ``x`` = ``MLP_MA_DECODER.encode(level="stage3")`` it gives the bits of ``encode(level="gmlp")``."""
    c = x.shape[-1] if x.dim() >= 2 else 0
    n, c_in = _linrelu_train_checks(x, weight, ((bias, "bias", (2 * c,)),))
    dev = x.device
    y = torch.empty(tuple(x.shape[:-1]) + (2 * c_in,), dtype=torch.float32, device=dev)
    launch("balf_linrelu_train_forward", dev, x, weight, bias, n, c_in, y)
    return LinreluTrainForward(y)


def linrelu_train_backward(g: torch.Tensor, y: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, want_dx=False) -> LinreluTrainBackward:
    """The backward of ``linrelu_train_forward`` (balf_linrelu_train_backward): ``g`` the total gradient at ``y``, ``y`` that
    forward's output (the ReLU's derivative is taken from it) -> the gradients of ``weight`` and ``bias`` and, with ``want_dx``, of
    ``x`` (``want_dx`` may be a contiguous float32 tensor of x's shape to write into)."""
    dx = want_dx if isinstance(want_dx, torch.Tensor) else None
    wide = tuple(x.shape[:-1]) + (2 * x.shape[-1],) if x.dim() >= 2 else None
    n, c_in = _linrelu_train_checks(x, weight, ((g, "g", wide), (y, "y", wide), (dx, "dx", tuple(x.shape))))
    dev = x.device
    l = lib()
    if dx is None and want_dx:
        dx = torch.empty_like(x)
    dw = torch.empty((2 * c_in, c_in), dtype=torch.float32, device=dev)
    db = torch.empty((2 * c_in,), dtype=torch.float32, device=dev)
    ws = _workspace("linrelu_train", dev, l.balf_linrelu_train_workspace_bytes(n, c_in))
    launch("balf_linrelu_train_backward", dev, g, y, x, weight, n, c_in, dw, db, dx, Workspace(ws))
    return LinreluTrainBackward(dw, db, dx)


class OptimArgumentError(BalfHipError, ValueError):
    """A tensor handed to the optimiser step is not what the kernel takes (also a ValueError: torch's optimisers raise that)."""


class OptimPointers:
    """What balf_adam_step / balf_sgd_step take of up to ``_lib.OPTIM_MAX_TENSORS`` parameters, gathered once and kept by the caller
    across steps: the host arrays of the parameters' (and, for Adam, the two moments') device pointers and element counts, and the
    array that each step fills with that step's gradient pointers.  ``key``: the ``data_ptr`` of every tensor it was made of -- a
    holder compares it to know when to gather again."""
    __slots__ = ("n", "device", "index", "numels", "key", "p", "m", "v", "numel", "g")


def _optim_tensor_check(t, name: str, dev, numel=None) -> None:
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
        raise OptimArgumentError(f"{name} must be a dense tensor (sparse gradients are not supported)")
    if t.dtype != torch.float32:
        raise OptimArgumentError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise OptimArgumentError(f"{name} must be contiguous")
    if t.device != dev:
        raise OptimArgumentError(f"{name} is on {t.device}, params[0] on {dev}")
    if numel is not None and t.numel() != numel:
        raise OptimArgumentError(f"{name} has {t.numel()} elements, its parameter {numel}")


def optim_pointers(params, exp_avgs=None, exp_avg_sqs=None) -> OptimPointers:
    """Check and gather 1..64 parameters (and their moments: both lists or neither) -> :class:`OptimPointers`.  Every tensor is
    float32, contiguous and on the GPU of ``params[0]``; a moment has its parameter's element count."""
    n = len(params)
    adam = exp_avgs is not None
    if (exp_avg_sqs is not None) != adam:
        raise BalfHipError("optim_pointers: give both moment lists or neither")
    if not 1 <= n <= _lib.OPTIM_MAX_TENSORS or (adam and not len(exp_avgs) == len(exp_avg_sqs) == n):
        raise BalfHipError(f"optim_pointers: 1..{_lib.OPTIM_MAX_TENSORS} parameters and as many of each moment, got {n}")
    dev = params[0].device if isinstance(params[0], torch.Tensor) else None
    for i, t in enumerate(params):
        _optim_tensor_check(t, f"params[{i}]", dev)
    for name, ts in (("exp_avgs", exp_avgs), ("exp_avg_sqs", exp_avg_sqs)):
        for i, t in enumerate(ts or ()):
            _optim_tensor_check(t, f"{name}[{i}]", dev, params[i].numel())
    require_gpu_tensor(params[0], "params[0]")
    o = OptimPointers()
    o.n, o.device, o.index = n, dev, params[0].get_device()
    o.numels = tuple(t.numel() for t in params)
    lists = (params, exp_avgs, exp_avg_sqs) if adam else (params,)
    o.key = tuple(t.data_ptr() for ts in lists for t in ts)
    arr = C.c_void_p * n
    o.p = arr(*o.key[:n])
    o.m = arr(*o.key[n:2 * n]) if adam else None
    o.v = arr(*o.key[2 * n:]) if adam else None
    o.numel = (C.c_int64 * n)(*o.numels)
    o.g = arr()
    return o


_F32, _STRIDED = torch.float32, torch.strided


def _optim_gradients(o: OptimPointers, grads) -> None:
    """This step's gradient pointers into ``o.g``; None (the parameter is skipped) as NULL.  This loop is most of what a step costs
    the host: one look per property, the message made only when one fails."""
    if len(grads) != o.n:
        raise BalfHipError(f"{len(grads)} gradients for {o.n} parameters")
    garr, numels, index = o.g, o.numels, o.index
    for i, g in enumerate(grads):
        if g is None:
            garr[i] = None
        elif (g.dtype is _F32 and g.layout is _STRIDED and g.get_device() == index and g.numel() == numels[i]
              and g.is_contiguous()):
            garr[i] = g.data_ptr()
        else:
            _optim_tensor_check(g, f"grads[{i}]", o.device, numels[i])
            raise BalfHipError(f"grads[{i}] is not what the kernel takes")        # (not reached: the check above names the reason)


def _optim_runs(n: int):
    return [(at, min(n, at + _lib.OPTIM_MAX_TENSORS)) for at in range(0, n, _lib.OPTIM_MAX_TENSORS)]


def adam_step(params, grads, exp_avgs, exp_avg_sqs, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
              step: int, pointers: Optional[OptimPointers] = None) -> None:
    """One step of ``torch.optim.Adam`` (amsgrad=False, maximize=False, L2 weight decay) in place on lists of tensors, ONE launch per
    64 tensors (balf_adam_step in include/balf_hip.h).  ``grads[i]`` None skips parameter i: it and its moments keep their bits.
    ``step`` is the number of this step (1 for the first) and is shared by all the tensors.  Every tensor is float32, contiguous and
    on one GPU, a gradient and the moments have their parameter's element count; lists longer than 64 are split into several calls.
    ``pointers``: :func:`optim_pointers` of exactly these parameters and moments (at most 64), kept by the caller across steps --
    then only the gradients are looked at."""
    if pointers is not None:
        if len(params) != pointers.n or pointers.m is None:
            raise BalfHipError("adam_step: pointers were not gathered from these lists")
        runs = ((pointers, grads),)
    else:
        if not len(params) == len(grads) == len(exp_avgs) == len(exp_avg_sqs) or not params:
            raise BalfHipError("adam_step: four non-empty lists of one length")
        runs = [(optim_pointers(params[a:b], exp_avgs[a:b], exp_avg_sqs[a:b]), grads[a:b]) for a, b in _optim_runs(len(params))]
    fn = lib().balf_adam_step
    step = int(step)
    for o, gs in runs:
        _optim_gradients(o, gs)
        check(on_device(o.index, lambda stream: fn(o.n, o.p, o.g, o.m, o.v, o.numel, lr, beta1, beta2, eps, weight_decay, step, stream)),
              "balf_adam_step")


def sgd_step(params, grads, lr: float, pointers: Optional[OptimPointers] = None) -> None:
    """``p -= lr * g`` in place on lists of tensors, one launch per 64 tensors (balf_sgd_step); the rules of :func:`adam_step`."""
    if pointers is not None:
        if len(params) != pointers.n:
            raise BalfHipError("sgd_step: pointers were not gathered from these lists")
        runs = ((pointers, grads),)
    else:
        if len(params) != len(grads) or not params:
            raise BalfHipError("sgd_step: two non-empty lists of one length")
        runs = [(optim_pointers(params[a:b]), grads[a:b]) for a, b in _optim_runs(len(params))]
    fn = lib().balf_sgd_step
    for o, gs in runs:
        _optim_gradients(o, gs)
        check(on_device(o.index, lambda stream: fn(o.n, o.p, o.g, o.numel, lr, stream)), "balf_sgd_step")
