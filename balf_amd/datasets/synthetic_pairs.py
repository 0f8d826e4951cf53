"""The synthetic-homography image pairs of the validation and of the training task, synthesised on the GPU (reference
balf/datasets/COCO.py:42-205; GOPRO inherits it): the loader that ``utils.train_utils.check_val_repeatability`` and
``utils.train_utils.train_head`` consume.

Per pair the reference warps the whole photograph with ``cv2.warpPerspective``, scatters the labels into two full-size heat
maps and cuts a window out of each of the four arrays, one pair per worker process.  Here the random geometry is drawn on the
host (``dataset_utils.sample_pair_geometry``: the reference's draws in the reference's order) and ``balf_synth_pairs``
(include/balf_hip.h) computes only the windows, ``batch_pairs`` pairs per call.

The training task (COCO.py:70-75, ``task == 'train'``) warps ``bgr_photometric_to_rgb(src_BGR)`` instead of the image: a random
brightness / contrast / saturation / hue / channel-order change between the two views.  ``photometric_seed`` selects it: the
parameters are drawn on the host (``dataset_utils.sample_photometric``, one set per homography draw, as the reference's loop
consumes them) and ``balf_synth_train_pairs`` distorts the taps of the destination window only; the distorted image is never
formed either.  The two cv2 colour conversions inside are defined by OpenCV's scalar 8-bit code; parity with cv2 itself is
unpinned.

Deviations from the reference, both deliberate:

* The reference redraws a homography whose WHOLE warped image is black (``dst_RGB.max() > 0``, COCO.py:77).  The full image
  is never formed here and nothing is redrawn; the largest 8-bit value of each destination PATCH is returned on the device
  instead (``SyntheticPairs.last_dst_max``, 0 = an all-black patch).
* The file walker and the image decoding are not ported: images (RGB) and labels are handed in.

The warp is defined as OpenCV's 8-bit INTER_LINEAR remap is documented; parity with cv2 itself is unpinned."""
from __future__ import annotations

import random

import numpy as np
import torch

from .. import ops
from . import dataset_utils


class SyntheticPairs:
    """An iterable over one pair per image: ``images_u8`` a list of uint8 RGB ``[H,W,3]`` arrays (sizes may differ), ``labels``
    the list of their ``[N,3]`` label rows (x, y, prob), ``hom_config`` the reference's ``config['homographic']`` dict
    (``perspective``, ``rotation``, ``scale``), ``patch_size`` the FINAL window (the validation task passes twice its
    configured patch size, as COCO.py:47; the training task the patch size itself, :44), ``top_k`` as ``select_k_best`` (0 keeps
    all), ``seed`` of the ``random.Random`` every geometry draw comes from (each ``iter()`` starts from it again: an epoch is
    reproducible).  ``photometric_seed`` None is the validation task; an int the training task: each ``iter()`` seeds a
    ``np.random.RandomState`` with it, the destination patch is that of the distorted image, and ``last_photometric`` holds the
    most recent call's ``sample_photometric`` results, one per pair.

    Yields, per pair, the reference loader's 6-tuple with a leading batch dimension of 1 -- ``images_src`` / ``images_dst``
    ``[1,3,p,p]``, ``heatmap_src`` / ``heatmap_dst`` ``[1,1,p,p]``, ``h_src_2_dst`` / ``h_dst_2_src`` ``[1,3,3]``, float32 --
    as views of device tensors that hold ``batch_pairs`` pairs from one ``balf_synth_pairs`` call.  Images and labels are
    uploaded once, at construction.  ``last_dst_max`` is the int32 device tensor of the most recent call (see the module
    docstring: nothing is redrawn for a black destination)."""

    def __init__(self, images_u8, labels, hom_config, patch_size, top_k, seed, batch_pairs=64, device=None, photometric_seed=None):
        if len(images_u8) == 0 or len(images_u8) != len(labels):
            raise ValueError("SyntheticPairs needs as many label arrays as images, and at least one")
        arrs = [np.ascontiguousarray(im) for im in images_u8]
        for a in arrs:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < patch_size or a.shape[1] < patch_size:
                raise ValueError(f"images must be uint8 [H,W,3] arrays of at least {patch_size} x {patch_size}, got {a.dtype} "
                                 f"{a.shape}")
        rows = [np.asarray(l, dtype=np.float32).reshape(-1, 3) for l in labels]
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.hom_config, self.patch_size, self.top_k, self.seed = dict(hom_config), int(patch_size), int(top_k), seed
        self.batch_pairs = max(1, int(batch_pairs))
        self.shapes = [a.shape for a in arrs]
        sizes = np.asarray([a.shape[:2] for a in arrs], dtype=np.int32)
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        pts_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        dev = self.device
        self._packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev)
        self._offsets, self._sizes = torch.from_numpy(offsets).to(dev), torch.from_numpy(sizes).to(dev)
        self._pts = torch.from_numpy(np.concatenate(rows) if rows else np.zeros((0, 3), np.float32)).to(dev)
        self._pts_off = torch.from_numpy(pts_off).to(dev)
        self.photometric_seed = None if photometric_seed is None else int(photometric_seed)
        self.last_dst_max = None
        self.last_photometric = None

    def __len__(self):
        return len(self.shapes)

    def synthesise(self, first, geometry):
        """One ``balf_synth_pairs`` call for the images ``first .. first + len(geometry) - 1`` with the given
        ``sample_pair_geometry`` results -> (img_src, img_dst, heat_src, heat_dst, h_src_2_dst, h_dst_2_src) device tensors.
        Geometry that carries ``"photometric"`` (every entry, or none) goes through ``balf_synth_train_pairs``."""
        n, dev = len(geometry), self.device
        host = np.concatenate([np.stack([g["inv_h"] for g in geometry]).reshape(n, 9),
                               np.asarray([g["win_src"] + g["win_dst"] for g in geometry], np.float64)], axis=1)
        train = "photometric" in geometry[0]
        if train:                                                # (perm rides along as a float64: 0..5 is exact)
            host = np.concatenate([host, np.stack([np.append(g["photometric"]["params"], g["photometric"]["perm"])
                                                   for g in geometry])], axis=1)
        t = torch.from_numpy(host).to(dev)                       # one upload for the matrices, the windows and the parameters
        wins = t[:, 9:13].to(torch.int32)
        hs = torch.from_numpy(np.stack([np.stack([g["h_src_2_dst"], g["h_dst_2_src"]]) for g in geometry])).to(dev)
        args = (self._packed, self._offsets[first:first + n], self._sizes[first:first + n], t[:, :9].contiguous(),
                wins[:, :2].contiguous(), wins[:, 2:].contiguous(), self._pts, self._pts_off[first:first + n + 1], self.top_k,
                self.patch_size)
        if train:
            img_s, img_d, heat_s, heat_d, dst_max = ops.synth_train_pairs(*args, t[:, 13:18].contiguous(),
                                                                          t[:, 18].to(torch.int32).contiguous())
        else:
            img_s, img_d, heat_s, heat_d, dst_max = ops.synth_pairs(*args)
        self.last_dst_max = dst_max
        self.last_photometric = [g["photometric"] for g in geometry] if train else None
        return img_s, img_d, heat_s, heat_d, hs[:, 0], hs[:, 1]

    def __iter__(self):
        rng = random.Random(self.seed)
        photometric_rng = None if self.photometric_seed is None else np.random.RandomState(self.photometric_seed)
        for first in range(0, len(self), self.batch_pairs):
            geometry = [dataset_utils.sample_pair_geometry(self.shapes[i], self.hom_config, self.patch_size, rng,
                                                           photometric_rng=photometric_rng)
                        for i in range(first, min(len(self), first + self.batch_pairs))]
            out = self.synthesise(first, geometry)
            for p in range(len(geometry)):
                yield tuple(t[p:p + 1] for t in out)
