"""The pre-processing of the resize protocol of the HSequences evaluation (reference balf/datasets/dataset_utils.py:15-60):
``ratio_preserving_resize`` on the GPU (``balf_resize_crop_u8``, include/balf_hip.h) and ``adapt_homography_to_preprocessing``
on the host.  The dataset walker ``Resize_HSequences`` (it reads files with cv2) is not ported.

PARITY of the resize is UNPINNED: the reference resizes with ``cv2.resize`` and crops with imgaug, neither of which is
available where this library is built.  The 8-bit arithmetic is defined in include/balf_hip.h after OpenCV's documented
INTER_LINEAR scheme and has not been checked against a cv2 build."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def adapt_homography_to_preprocessing(zip_data, args):
    """The homography between the two RESIZED images, bit-identical to the reference (host, NumPy): ``zip_data`` holds
    ``'homography'`` (source -> destination of the original images), ``'shape'`` and ``'warped_shape'`` (H, W arrays of the
    two originals); ``args.resize_shape`` is the target (H, W).  Sizes and target are taken as float32, as there; the crop
    offsets are floored (``// 2.0``)."""
    h = zip_data['homography'].astype(np.float32)
    size_src = zip_data['shape'].astype(np.float32)
    size_dst = zip_data['warped_shape'].astype(np.float32)
    target = np.array(args.resize_shape, dtype=np.float32)
    # resized source pixel -> original source pixel: undo the crop, then the scale
    s_src = np.max(target / size_src)
    crop_y, crop_x = (size_src * s_src - target) // 2.0
    uncrop = np.array([[1, 0, crop_x], [0, 1, crop_y], [0, 0, 1]], dtype=np.float32)
    unscale = np.diag([1. / s_src, 1. / s_src, 1])
    # original destination pixel -> resized destination pixel: the scale, then the crop
    s_dst = np.max(target / size_dst)
    scale = np.diag([s_dst, s_dst, 1])
    crop_y, crop_x = (size_dst * s_dst - target) // 2.0
    crop = np.array([[1, 0, -crop_x], [0, 1, -crop_y], [0, 0, 1]], dtype=np.float32)
    return crop @ scale @ h @ unscale @ uncrop


def ratio_preserving_resize_batch(images, target_size, device=None) -> torch.Tensor:
    """``ratio_preserving_resize`` of a list of uint8 images of different sizes -- all gray ``[H,W]`` or all 3-channel
    ``[H,W,3]``, NumPy arrays or tensors -- in ONE launch -> a uint8 device tensor ``[B,th,tw]`` / ``[B,th,tw,3]``, the input of
    ``pipeline.detect_batch_u8``.  The images are packed back to back on the host and uploaded once.  Channel order is kept."""
    if len(images) == 0:
        raise ValueError("ratio_preserving_resize_batch needs at least one image")
    arrs = [im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im) for im in images]
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
            raise ValueError(f"images must be non-empty uint8 [H,W], [H,W,1] or [H,W,3] arrays, got {a.dtype} {a.shape}")
    chans = {1 if a.ndim == 2 else a.shape[2] for a in arrs}
    if len(chans) != 1:
        raise ValueError("gray and 3-channel images cannot share one batch")
    c = chans.pop()
    th, tw = int(target_size[0]), int(target_size[1])
    if th <= 0 or tw <= 0:
        raise ValueError(f"target_size must be positive, got {target_size}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    sizes = np.asarray([a.shape[:2] for a in arrs], dtype=np.int32)
    nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * c
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    packed = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in arrs])
    return ops.resize_crop_u8(torch.from_numpy(packed).to(dev), torch.from_numpy(offsets).to(dev),
                              torch.from_numpy(sizes).to(dev), c, th, tw)


def ratio_preserving_resize(img, target_size):
    """One uint8 image ``[H,W]`` / ``[H,W,3]`` (NumPy) -> the image scaled by ``max(th / H, tw / W)`` (bilinear) and centre
    cropped / zero padded to ``target_size`` (NumPy, same number of dimensions): the reference's signature, computed on the
    GPU by :func:`ratio_preserving_resize_batch`."""
    img = np.asarray(img)
    out = ratio_preserving_resize_batch([img], target_size)[0].cpu().numpy()
    return out[..., None] if img.ndim == 3 and img.shape[2] == 1 else out
