"""The pre-processing of the resize protocol of the HSequences evaluation (reference balf/datasets/dataset_utils.py:15-60):
``ratio_preserving_resize`` on the GPU (``balf_resize_crop_u8``, include/balf_hip.h) and ``adapt_homography_to_preprocessing``
on the host.  The dataset walker ``Resize_HSequences`` (it reads files with cv2) is not ported.

The geometry of the synthetic-homography pairs of the validation task (reference :137-192, :277-304 and COCO.py:97-142), on
the host -- 3 x 3 arithmetic per pair: ``generate_homography``, ``get_dst_point``, ``get_window_point``,
``sample_pair_geometry``, and ``select_k_best`` / ``labels_to_heatmap`` as NumPy restatements.  The per-pixel part (warp,
crops, heat maps) is ``balf_synth_pairs`` (datasets/synthetic_pairs.py).  The two cv2 calls of ``generate_homography`` are
written out (``getRotationMatrix2D`` in closed form, ``getPerspectiveTransform`` as the 8 x 8 float64 solve); their last
bits against a cv2 build are UNPINNED.

The photometric distortion of the TRAINING task (reference :10-12, :76-134): ``sample_photometric`` draws ``bgr_distorsion``'s
random numbers on the host, in its order and with its quirks, and ``balf_photometric_u8`` (whole images: ``bgr_distorsion``,
``bgr_photometric_to_rgb``) or ``balf_synth_train_pairs`` (only the destination window, datasets/synthetic_pairs.py) applies
them.  The two cv2 colour conversions are defined in include/balf_hip.h by OpenCV's scalar 8-bit code; parity with a cv2 build
is UNPINNED.

PARITY of the resize is UNPINNED: the reference resizes with ``cv2.resize`` and crops with imgaug, neither of which is
available where this library is built.  The 8-bit arithmetic is defined in include/balf_hip.h after OpenCV's documented
INTER_LINEAR scheme and has not been checked against a cv2 build."""
from __future__ import annotations

import math
import random

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


# ---- the training task's photometric distortion -----------------------------------------------------------------------------
perms = ((0, 1, 2), (0, 2, 1),
         (1, 0, 2), (1, 2, 0),
         (2, 0, 1), (2, 1, 0))
PHOTOMETRIC_NEUTRAL = (0.0, 1.0, 1.0, 0.0, 1.0)


def sample_photometric(rng=None, lower=.5, upper=1.5, delta=18.0, delta_brigtness=36):
    """The random numbers of one ``bgr_distorsion`` call (reference :81-121), from ``np.random`` or the ``RandomState`` passed
    as ``rng``, in the reference's order: a coin before every step, its value only when the coin fell.  -> dict ``params``
    float64 [5] = (delta_b, alpha1, sat, hue, alpha2) and ``perm`` (a row of ``perms``); a step that did not fire has its
    neutral value (``PHOTOMETRIC_NEUTRAL``, perm 0), which makes it the identity bit for bit.  The reference's quirks are
    kept: the brightness branch OVERWRITES ``delta``, so the hue is then drawn from ``uniform(-brightness, brightness)``; the
    second contrast gain is drawn only when the first was."""
    rng = np.random if rng is None else rng
    delta_b = 0.0
    if rng.randint(2):
        delta = rng.uniform(-delta_brigtness, delta_brigtness)
        delta_b = delta
    contrast = rng.randint(2)
    alpha1 = rng.uniform(lower, upper) if contrast else 1.0
    sat = rng.uniform(lower, upper) if rng.randint(2) else 1.0
    hue = rng.uniform(-delta, delta) if rng.randint(2) else 0.0
    alpha2 = rng.uniform(lower, upper) if contrast else 1.0
    perm = int(rng.randint(len(perms))) if rng.randint(2) else 0
    return {"params": np.array([delta_b, alpha1, sat, hue, alpha2], dtype=np.float64), "perm": perm}


def photometric_u8(image, photometric, blue_idx=0):
    """One uint8 ``[H,W,3]`` NumPy image through ``balf_photometric_u8`` with a ``sample_photometric`` result -> NumPy."""
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
        raise ValueError(f"image must be a non-empty uint8 [H,W,3] array, got {image.dtype} {image.shape}")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = ops.photometric_u8(torch.from_numpy(image.reshape(-1)).to(dev), torch.zeros(1, dtype=torch.int64, device=dev),
                             torch.tensor([image.shape[:2]], dtype=torch.int32, device=dev),
                             torch.from_numpy(np.asarray(photometric["params"], np.float64).reshape(1, 5)).to(dev),
                             torch.tensor([photometric["perm"]], dtype=torch.int32, device=dev), blue_idx)
    return out.cpu().numpy().reshape(image.shape)


def bgr_distorsion(image, lower=0.5, upper=1.5, delta=18.0, delta_brigtness=36):
    """The reference's signature: a uint8 BGR ``[H,W,3]`` NumPy image -> its random photometric distortion (NumPy, uint8),
    the draws from ``np.random`` (``sample_photometric``), the pixels on the GPU."""
    return photometric_u8(image, sample_photometric(None, lower, upper, delta, delta_brigtness))


def bgr_photometric_to_rgb(im_bgr):
    """Reference :76-79: ``bgr_distorsion``, then the channels reversed."""
    img_rgb = np.ascontiguousarray(bgr_distorsion(im_bgr)[:, :, ::-1])
    return img_rgb.reshape(img_rgb.shape[0], img_rgb.shape[1], 3)


def check_margins(img, axis=-1):
    """Reference :123-130: clamp a float image (``axis`` -1) or one of its channels to [0, 255], in place; returns it."""
    view = img if axis == -1 else img[:, :, axis]
    view[view > 255.0] = 255.0
    view[view < 0.0] = 0.0
    return img


def swap_channels(image, swaps):
    """Reference :132-134: the channels of ``image`` in the order ``swaps``."""
    return image[:, :, swaps]


# ---- synthetic-homography pairs: the host side ------------------------------------------------------------------------------
def get_dst_point(perspective, IMAGE_SHAPE, rng=None):
    """The four perturbed corners (float32 [4,3], homogeneous), reference :161-192: seven ``random()`` draws in its order."""
    rng = random if rng is None else rng
    a, b, c, d, e, f = (rng.random() for _ in range(6))
    if rng.random() > 0.5:
        lt, rt = (perspective * a, perspective * b), (0.9 + perspective * c, perspective * d)
        lb, rb = (perspective * a, 0.9 + perspective * e), (0.9 + perspective * c, 0.9 + perspective * f)
    else:
        lt, rt = (perspective * a, perspective * b), (0.9 + perspective * c, perspective * d)
        lb, rb = (perspective * e, 0.9 + perspective * b), (0.9 + perspective * f, 0.9 + perspective * d)
    return np.array([(IMAGE_SHAPE[1] * x, IMAGE_SHAPE[0] * y, 1) for x, y in (lt, rt, lb, rb)], dtype='float32')


def rotation_matrix_2d(center, angle, scale):
    """``cv2.getRotationMatrix2D`` in closed form (float64 [2,3]; the centre is taken as float32, as cv2's Point2f)."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    alpha, beta = math.cos(angle * math.pi / 180.0) * scale, math.sin(angle * math.pi / 180.0) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


def perspective_transform(src, dst):
    """``cv2.getPerspectiveTransform`` of four point pairs (float32 [4,2]): OpenCV's 8 x 8 system solved in float64, the last
    element 1.  Last bits against cv2 (its own LU) are unpinned."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    a, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y = src[i]
        a[i] = (x, y, 1, 0, 0, 0, -x * dst[i, 0], -y * dst[i, 0])
        a[i + 4] = (0, 0, 0, x, y, 1, -x * dst[i, 1], -y * dst[i, 1])
        b[i], b[i + 4] = dst[i]
    return np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)


def generate_homography(IMAGE_SHAPE, hom_config, rng=None):
    """Reference :137-159: a random perspective + rotation + scale about a jittered centre, float64 [3,3].  Consumes the
    ``random`` module (or the ``random.Random`` passed as ``rng``) in the reference's call order: ``get_dst_point``'s seven
    draws, then four ``randint`` (rotation, scale, centre x, centre y)."""
    rng = random if rng is None else rng
    src_point = np.array([[0, 0], [IMAGE_SHAPE[1] - 1, 0], [0, IMAGE_SHAPE[0] - 1], [IMAGE_SHAPE[1] - 1, IMAGE_SHAPE[0] - 1]],
                         dtype=np.float32)
    dst_point = get_dst_point(hom_config['perspective'], IMAGE_SHAPE, rng)
    rotation = hom_config['rotation']
    rot = rng.randint(-rotation, rotation)
    scale = 1.0 + hom_config['scale'] * rng.randint(-25, 50) * 0.1
    center_offset = 40
    center = (IMAGE_SHAPE[1] / 2 + rng.randint(-center_offset, center_offset),
              IMAGE_SHAPE[0] / 2 + rng.randint(-center_offset, center_offset))
    rs_mat = rotation_matrix_2d(center, rot, scale)
    f_point = np.matmul(dst_point, rs_mat.T).astype('float32')
    return perspective_transform(src_point, f_point)


def get_window_point(shape, patch_size, crop_type='random', rng=None):
    """Reference :295-304: the centre (row, col) of the source window.  The reference hands ``patch_size / 2`` (a float) to
    ``randint``; here the bounds are converted to int first (the same draws for an even ``patch_size``)."""
    rng = random if rng is None else rng
    h, w = shape[0], shape[1]
    if crop_type == 'random':
        window_h = rng.randint(int(patch_size / 2), int(h - patch_size / 2))
        window_w = rng.randint(int(patch_size / 2), int(w - patch_size / 2))
    else:
        window_h, window_w = h / 2, w / 2
    return np.array([window_h, window_w])


def select_k_best(points, k):
    """Reference :277-286 restated: the ``k`` rows of largest prob (all for ``k == 0`` or fewer rows), in ascending prob.  Ties
    at the cut keep the LOWER row index, the rule of ``balf_synth_pairs`` (the reference's argsort is unstable there)."""
    points = np.asarray(points)
    if points.shape[1] > 2 and k != 0:
        order = np.argsort(-points[:, 2], kind="stable")[:min(k, points.shape[0])]
        return points[order[::-1]]
    return points


def labels_to_heatmap(points, IMAGE_SHAPE):
    """Reference :288-292: float32 [H,W], 1 at the truncated (y, x) of every point."""
    heatmap = np.zeros((IMAGE_SHAPE[0], IMAGE_SHAPE[1]))
    points = np.asarray(points).astype(int)
    heatmap[points[:, 1], points[:, 0]] = 1
    return heatmap.astype('float32')


def compose_pair_homographies(h, point_src, point_dst, patch_size):
    """COCO.py:111-116 and :135-142: the homographies between the two PATCHES -> (h_src_2_dst, h_dst_2_src) float32 [3,3]:
    float64 ``np.dot`` / ``np.linalg.inv``, then the float32 cast, then the division by [2,2]."""
    h_src_translation = np.asanyarray([[1., 0., -(int(point_src[1]) - patch_size / 2)],
                                       [0., 1., -(int(point_src[0]) - patch_size / 2)],
                                       [0., 0., 1.]])
    h_dst_translation = np.asanyarray([[1., 0., int(point_dst[1] - patch_size / 2)],
                                       [0., 1., int(point_dst[0] - patch_size / 2)],
                                       [0., 0., 1.]])
    homography = np.dot(h_src_translation, np.dot(h, h_dst_translation))
    h_dst_2_src = homography.astype('float32')
    h_dst_2_src = h_dst_2_src / h_dst_2_src[2, 2]
    h_src_2_dst = np.linalg.inv(homography).astype('float32')
    h_src_2_dst = h_src_2_dst / h_src_2_dst[2, 2]
    return h_src_2_dst, h_dst_2_src


def sample_pair_geometry(shape, hom_config, patch_size, rng=None, max_draws=10000, photometric_rng=None):
    """The random part of one pair of the reference's loader (COCO.py:53-142) for an image of ``shape`` (h, w[, c]): draw a
    homography, the source window, map its centre with ``inv_h``; a destination window that leaves the image redraws the pair
    FROM THE HOMOGRAPHY ON, as the reference's loop does.  -> dict: ``inv_h`` float64 [3,3] (what ``cv2.warpPerspective`` is
    handed), ``win_src`` / ``win_dst`` (top row, left column) ints, ``h_src_2_dst`` / ``h_dst_2_src`` float32 [3,3].
    Not reproduced: the reference also redraws a homography whose whole warped image is black (see SyntheticPairs).
    ``photometric_rng`` (a ``np.random.RandomState``) selects the training task: EVERY homography draw of the loop is followed
    by one ``sample_photometric(photometric_rng)`` -- the reference distorts inside its loop, so a redraw consumes a set -- and
    the accepted draw's set is returned under ``"photometric"``.  Without it nothing changes: the same draws, the same dict."""
    rng = random if rng is None else rng
    half = patch_size / 2
    if shape[0] < patch_size or shape[1] < patch_size:
        raise ValueError(f"an image of {tuple(shape[:2])} holds no {patch_size} x {patch_size} window")
    for _ in range(max_draws):
        h = generate_homography(shape, hom_config, rng)
        inv_h = np.linalg.inv(h)
        inv_h = inv_h / inv_h[2, 2]
        photometric = None if photometric_rng is None else sample_photometric(photometric_rng)
        point_src = get_window_point(shape, patch_size, rng=rng)
        point_dst = inv_h.dot([point_src[1], point_src[0], 1.0])
        point_dst = [point_dst[1] / point_dst[2], point_dst[0] / point_dst[2]]
        if (point_dst[0] - half) < 0 or (point_dst[1] - half) < 0:
            continue
        if (point_dst[0] + half) > shape[0] or (point_dst[1] + half) > shape[1]:
            continue
        win_src = (int(point_src[0] - half), int(point_src[1] - half))
        win_dst = (int(point_dst[0] - half), int(point_dst[1] - half))
        if any(int(c + half) - int(c - half) != patch_size for c in point_dst):     # the reference's final shape check
            continue
        h_src_2_dst, h_dst_2_src = compose_pair_homographies(h, point_src, point_dst, patch_size)
        out = {"inv_h": inv_h, "win_src": win_src, "win_dst": win_dst, "h_src_2_dst": h_src_2_dst, "h_dst_2_src": h_dst_2_src}
        if photometric is not None:
            out["photometric"] = photometric
        return out
    raise RuntimeError(f"no destination window inside the image in {max_draws} draws: {hom_config} on {tuple(shape[:2])}")
