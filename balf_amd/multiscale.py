"""Multi-scale keypoint extraction over an image pyramid: the HSequences detection protocol that the reference configures
(balf/configs/config_hpatches.py:50-80, ``parse_multiscale_config``: scale_factor_levels, pyramid_levels,
upsampled_levels, num_points, nms_size, border_size) but ships no driver for.  This module is its specification
(multi-scale extraction); everything after the host-side plan runs on the GPU, stream-ordered:

1. Levels ``i = 0 .. L-1`` of scale ``s_i = r ** (i - U)``: level U is the input (as the forward's prepared input), the
   levels below it are level U resized bilinearly to ``floor(h f + 0.5)`` with ``f = r ** (U - i)``, each level above it
   is the level before blurred (Gaussian, sigma = 2r/6, radius int(4 sigma + 0.5), half-sample symmetric border) and
   resized to ``ceil(h / r)``.  A level whose smaller side would be <= 2 border_size ends the pyramid.
2. Each level through the forward, then crop / border / window NMS / top-K as ``balf_nms_topk`` with K from a point
   budget: ``point_level[i] = int(N (r^2)^-(i-U) / sum_j (r^2)^-(j-U))``, ``K_i = sum_{a<=i} point_level[a] - (points
   taken by levels < i)``, clamped to h_i w_i -- decided on the device per image.
3. The level lists mapped through ``H_i = inv(diag(1/s_i, 1/s_i, 1))`` with the arithmetic of apply_homography_to_points
   (the third column becomes the radius compute_repeatability reads), ordered by (score desc, level asc, index asc),
   truncated to N; ``order_coord='yxsr'`` swaps the first two columns.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

from . import _lib, arch, ops
from .guard import run_guarded


@dataclass
class PyramidPlan:
    shapes: List[Tuple[int, int]]                  # (h_i, w_i) of the built levels
    padded: List[Tuple[int, int, int, int]]        # (Hp, Wp, top, left) of each level (arch.padded_hw)
    scales: List[float]                            # s_i = r ** (i - U)
    homographies: List[np.ndarray]                 # H_i, 3x3 float64: level -> original image coordinates
    point_level: List[int]
    cum_budget: List[int]                          # sum_{a <= i} point_level[a]
    num_points: int
    upsampled_levels: int
    sigma: float                                   # blur of the levels above U


def pyramid_plan(h: int, w: int, num_points: int = 1500, scale_factor_levels: float = np.sqrt(2), pyramid_levels: int = 5,
                 upsampled_levels: int = 1, border_size: int = 15) -> PyramidPlan:
    """The host side of the protocol for an ``h x w`` input: level shapes, padding, scales, homographies, point budget."""
    r = float(scale_factor_levels)
    p, u, n = int(pyramid_levels), int(upsampled_levels), int(num_points)
    if not r > 1.0:
        raise ValueError(f"scale_factor_levels must be > 1, got {scale_factor_levels}")
    if p < 0 or u < 0:
        raise ValueError(f"pyramid_levels and upsampled_levels must be >= 0, got {pyramid_levels}, {upsampled_levels}")
    if n <= 0 or n > _lib.MAX_TOPK:
        raise ValueError(f"num_points must be in 1..{_lib.MAX_TOPK}, got {num_points}")
    if h <= 0 or w <= 0:
        raise ValueError(f"bad image size {h}x{w}")
    full: List[Tuple[int, int]] = [None] * (p + u + 1)
    full[u] = (int(h), int(w))
    for i in range(u - 1, -1, -1):
        f = r ** (u - i)
        full[i] = (int(math.floor(h * f + 0.5)), int(math.floor(w * f + 0.5)))
    for i in range(u + 1, p + u + 1):
        full[i] = (int(math.ceil(full[i - 1][0] / r)), int(math.ceil(full[i - 1][1] / r)))
    shapes = []
    for s in full:                                 # the first small level ends the pyramid
        if min(s) <= 2 * border_size:
            break
        shapes.append(s)
    if not shapes:
        raise ValueError(f"no pyramid level of a {h}x{w} image is larger than 2 * border_size = {2 * border_size}")
    if len(shapes) > _lib.MAX_PYRAMID_LEVELS:
        raise ValueError(f"{len(shapes)} levels: at most {_lib.MAX_PYRAMID_LEVELS} are supported")
    for hh, ww in shapes:
        hp, wp, _, _ = arch.padded_hw(hh, ww)
        if hp * wp > 1 << 25:
            raise ValueError(f"a {hh}x{ww} level pads to {hp}x{wp}: more than 2^25 pixels")
    nl = len(shapes)
    r2 = r ** 2
    tmp = sum(r2 ** -(i - u) for i in range(nl))
    point_level = [int(n * r2 ** -(i - u) / tmp) for i in range(nl)]
    scales = [r ** (i - u) for i in range(nl)]
    return PyramidPlan(shapes=shapes, padded=[arch.padded_hw(hh, ww) for hh, ww in shapes], scales=scales,
                       homographies=[np.linalg.inv(np.diag([1.0 / s, 1.0 / s, 1.0])) for s in scales],
                       point_level=point_level, cum_budget=list(np.cumsum(point_level).tolist()), num_points=n,
                       upsampled_levels=u, sigma=2.0 * r / 6.0)


def gaussian_taps(sigma: float) -> np.ndarray:
    """The blur's normalised taps, float64 (balf_pyramid_level rounds them to fp32)."""
    rad = int(4.0 * sigma + 0.5)
    k = np.arange(-rad, rad + 1, dtype=np.float64)
    t = np.exp(-0.5 * k * k / (sigma * sigma))
    return t / t.sum()


def _order_yx(order_coord: str) -> bool:
    if order_coord not in ("xysr", "yxsr"):
        raise ValueError(f"order_coord must be 'xysr' or 'yxsr', got {order_coord!r}")
    return order_coord == "yxsr"


def detect_levels(model, levels, plan: PyramidPlan, border_size: int = 15, nms_size: int = 15):
    """Forward + budgeted top-K of every level -> (idx [L,B,N], score [L,B,N], count [L,B]), all on the device."""
    nl, b, n = len(levels), levels[0].shape[0], plan.num_points
    dev = levels[0].device
    idx = torch.empty((nl, b, n), dtype=torch.int32, device=dev)
    score = torch.empty((nl, b, n), dtype=torch.float32, device=dev)
    count = torch.empty((nl, b), dtype=torch.int32, device=dev)
    taken = torch.zeros((b,), dtype=torch.int32, device=dev)
    for i, x in enumerate(levels):
        prob = model(x, want_logits=False)["prob"]
        hh, ww = plan.shapes[i]
        _, _, top, left = plan.padded[i]
        ops.nms_topk_budget(prob, top, left, hh, ww, border_size, nms_size, plan.cum_budget[i], n, taken,
                            idx[i], score[i], count[i])
    return idx, score, count


def _detect(model, images: torch.Tensor, num_points, border_size, nms_size, scale_factor_levels, pyramid_levels,
            upsampled_levels, order_coord):
    order_yx = _order_yx(order_coord)
    plan = pyramid_plan(images.shape[1], images.shape[2], num_points, scale_factor_levels, pyramid_levels, upsampled_levels,
                        border_size)
    levels = ops.build_pyramid(images, plan.shapes, plan.upsampled_levels, plan.sigma)
    idx, score, count = detect_levels(model, levels, plan, border_size, nms_size)
    return ops.multiscale_merge(idx, score, count, [s[1] for s in plan.shapes], plan.homographies, plan.num_points,
                                order_yx)


def detect_batch_multiscale_u8(model, images_u8: torch.Tensor, num_points: int = 1500, border_size: int = 15,
                               nms_size: int = 15, scale_factor_levels: float = np.sqrt(2), pyramid_levels: int = 5,
                               upsampled_levels: int = 1, order_coord: str = "xysr"):
    """uint8 gray ``[B,H,W]`` or RGB ``[B,H,W,3]`` images on the GPU -> (pts [B,N,4] float64, count [B] int32) on the GPU:
    rows ``(x, y, radius, score)`` (``yxsr``: y first) in original-image coordinates, sorted by score, rows past the count
    zero.  Nothing is read back (capturable with ``torch.cuda.graph``).  Split-f16 guard: as
    ``pipeline.detect_batch_u8`` -- ``model.fp16_guard_check()`` returns True when a level's forward was flagged."""
    if images_u8.dtype != torch.uint8:
        raise ValueError("images_u8 must be uint8 [B,H,W] or [B,H,W,3]")
    return _detect(model, images_u8, num_points, border_size, nms_size, scale_factor_levels, pyramid_levels,
                   upsampled_levels, order_coord)


def detect_batch_multiscale(model, images: torch.Tensor, num_points: int = 1500, border_size: int = 15, nms_size: int = 15,
                            scale_factor_levels: float = np.sqrt(2), pyramid_levels: int = 5, upsampled_levels: int = 1,
                            order_coord: str = "xysr"):
    """:func:`detect_batch_multiscale_u8` for float images ``[B,H,W,3]`` in [0, 1] on the GPU (cast to float32 first)."""
    if not images.is_floating_point():
        raise ValueError("images must be a float [B,H,W,3] tensor")
    return _detect(model, images, num_points, border_size, nms_size, scale_factor_levels, pyramid_levels, upsampled_levels,
                   order_coord)


@torch.no_grad()
def extract_multiscale_detections(image_RGB_norm, model, device, nms_size=15, num_points=1500, border_size=15,
                                  scale_factor_levels=np.sqrt(2), pyramid_levels=5, upsampled_levels=1, order_coord="xysr"):
    """One ``[H,W,3]`` float image in [0, 1] on the host -> ``[n, 4]`` float64 rows (x, y, radius, score) (``yxsr``: y
    first), n <= num_points, sorted by score: what the HSequences extraction feeds ``compute_repeatability`` /
    ``apply_homography_to_points``.  Like ``pipeline.extract_detections``, a call whose split-f16 forward was flagged is
    repeated on the fp32 kernels before anything is returned (``guard.run_guarded``: one forward per level)."""
    img = np.ascontiguousarray(image_RGB_norm)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"expected an [H,W,3] image, got {img.shape}")
    if img.dtype not in (np.float64, np.float32, np.float16):
        img = img.astype(np.float64)
    x = torch.from_numpy(img).to(device)[None].to(torch.float32).contiguous()
    args = (num_points, border_size, nms_size, scale_factor_levels, pyramid_levels, upsampled_levels, order_coord)

    def run():
        pts, count = _detect(model, x, *args)
        return pts, int(count[0])      # (a device-to-host read: the stream has passed every level's forward)
    pts, n = run_guarded(model, run)
    return pts[0, :n].cpu().numpy()
