"""The inference / evaluation helpers of /root/reference/balf/utils/train_utils.py with every stage on the GPU.
Of training (``train_model``, train_utils.py:79-160) the head's part is here: ``train_head`` fits the trainable tail on the
features of the frozen encoder (:mod:`balf_amd.model.head_train`) against :mod:`balf_amd.loss.loss_function`; the encoder's
backward is out of scope.  The set-up of the reference's train.py is here too: ``build_optimizer`` (:mod:`balf_amd.optim`'s fused
Adam / SGD for GPU parameters), ``build_scheduler``, ``WarmRestart``, ``LinearDecay`` and ``ckpt_state`` (train_utils.py:20-76,
199-203); ``train_model`` itself is not.

* ``extract_detections`` (train_utils.py:416-454) -- see :mod:`balf_amd.pipeline`.
* ``compute_repeatability_with_maximum_filter`` (train_utils.py:170-196): window-max NMS of both score maps, common-
  region masks (supplied by the caller: the reference builds them with ``cv2.warpPerspective``, which is not rebuilt
  here), top-K points, homography of the destination points, repeatability.
* ``check_val_hsequences_repeatability`` (train_utils.py:308-413): the HSequences validation loop, with every image
  detected once and in batches and all pairs evaluated by the batched core (``benchmark_test.evaluate``).
* ``check_val_repeatability`` (train_utils.py:205-306): the per-epoch validation on synthetic-homography pairs that the
  reference selects checkpoints by (train.py:87,113), pairs forwarded in batches and both of its evaluations (greedy NMS
  and window NMS) run by the batched core from the same forward.  Its tensorboard logging is not ported.
* ``prob_to_score_maps_tensor_batch`` (train_utils.py:162-168): the maps that logging draws, ``apply_nms_fast`` of a batch in
  one call on the GPU.  The validations do not call it.
* ``check_val_anchor_loss``: the quantity ``train_model`` logs as ``total_loss`` (train_utils.py:104-120), evaluated over a
  validation loader without gradients.  The reference has no such function: it only sees the loss while training.
* ``train_head``: one epoch of ``train_model``'s step (train_utils.py:104-124) for the head alone, encoder frozen.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch

from ..benchmark_test import _chunked, evaluate, geometry_tools, repeatability_tools
from ..guard import run_guarded
from ..loss import loss_function
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


def prob_to_score_maps_tensor_batch(prob_outputs, nms_size):
    """``apply_nms_fast(prob_outputs[b], nms_size)`` for every map of ``prob_outputs`` [B,H,W] (float32, on the GPU) in one
    launch -> [B,1,H,W] float32 ON THE INPUT'S DEVICE.  The reference (train_utils.py:162-168) loops over the batch on the
    host and returns a CPU tensor: call ``.cpu()`` on the result where a host tensor is needed."""
    return repeatability_tools.nms_fast_score_map_batch(prob_outputs.detach(), nms_size).unsqueeze(1)


_REP_FIELDS = ('rep_single_scale', 'rep_multi_scale', 'error_overlap_single_scale', 'error_overlap_multi_scale',
               'possible_matches', 'num_points_single_scale', 'num_points_multi_scale', 'candidates_single_scale',
               'candidates_multi_scale')
_MEANS = _REP_FIELDS[:5]       # what both validations return the means of, in this order
_SEQ_COLUMNS = _REP_FIELDS + ('valid',)


def _evaluate_chunk(seqs, model, device, nms_size, num_points, border_size, multi_scale, batch_size):
    """Detect the images of some sequences and evaluate their pairs -> the _SEQ_COLUMNS on the host, one row per pair in
    (sequence, destination) order."""
    images, src_ids, dst_ids, hs, shapes = _chunked.chunk_pairs(seqs)
    if not src_ids:
        return _chunked.Table(_SEQ_COLUMNS)
    rows, count = _chunked.detect_images(images, model, device, nms_size, num_points, border_size, multi_scale, batch_size)
    s_at, d_at = _chunked.pair_index(src_ids, dst_ids, device)
    args = (rows[s_at], count[s_at], rows[d_at], count[d_at], torch.from_numpy(np.stack(hs)).to(device),
            torch.tensor(shapes, dtype=torch.int32, device=device))
    return _chunked.with_edge_retry(lambda **kw: _chunked.host_table(evaluate.evaluate_pairs(*args, **kw), _SEQ_COLUMNS))


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
    was flagged, or during which the checkpoint was switched to the fp32 kernels, is repeated (``guard.run_guarded``).
    ``multi_scale=True`` detects with ``multiscale.detect_batch_multiscale`` (``pyramid_plan`` defaults; ``num_points`` /
    ``nms_size`` / ``border_size`` as given), the multi-scale HSequences protocol, equal to the same loop over
    ``extract_multiscale_detections``.  ``tb_log`` must be None: the reference's image logging is not ported.
    ``cell_size`` and ``cur_epoch`` are unused, as in the reference."""
    if tb_log is not None:
        raise NotImplementedError("check_val_hsequences_repeatability: tensorboard image logging is not ported; pass tb_log=None")
    device = torch.device(device)
    chunk, batch_size = max(1, int(chunk_sequences)), max(1, int(batch_size))
    _, t = _chunked.run_sequence_chunks(dataloader, model, chunk, _SEQ_COLUMNS, lambda seqs: _evaluate_chunk(
        seqs, model, device, nms_size, num_points, border_size, multi_scale, batch_size))
    valid = t['valid'] != 0            # (the reference's loop skips a pair with an empty kept list)
    return tuple(t[k][valid].mean() for k in _MEANS)


_VAL_CONF_THRESH = 0.015      # get_nms_score_map_from_score_map(..., conf_thresh=0.015), train_utils.py:242-243


def _evaluate_val_chunk(pairs, model, device, nms_size, num_points, batch_size, max_edges=None):
    """``pairs``: (image_src [3,Hs,Ws], image_dst [3,Hd,Wd], h_dst_2_src [3,3]) tensors.  Forward them (pairs of one shape
    ``batch_size`` at a time) and evaluate both legs from that forward -> the _REP_FIELDS on the host, values [P, 2, 9] (leg 0
    greedy, leg 1 window)."""
    out = torch.zeros((len(pairs), 2, len(_REP_FIELDS)), dtype=torch.float64, device=device)
    kw = {} if max_edges is None else {"max_edges": int(max_edges)}
    for sel in _chunked.batches_by_shape(pairs, lambda p: (tuple(p[0].shape), tuple(p[1].shape)), batch_size):
        prob_src = model(torch.stack([pairs[i][0] for i in sel]).to(device), want_logits=False)["prob"]
        prob_dst = model(torch.stack([pairs[i][1] for i in sel]).to(device), want_logits=False)["prob"]
        h = torch.stack([pairs[i][2].reshape(3, 3) for i in sel]).to(device=device, dtype=torch.float64)
        at = torch.tensor(sel, dtype=torch.long, device=device)
        for leg_id, leg in enumerate(("greedy", "window")):
            r = evaluate.evaluate_val_pairs(prob_src, prob_dst, h, nms_size, num_points, leg=leg, conf_thresh=_VAL_CONF_THRESH,
                                            **kw)
            out[at, leg_id] = _chunked.stack_columns(r, _REP_FIELDS)
    return _chunked.Table(_REP_FIELDS, out.cpu().numpy())       # the one device-to-host read of the chunk


def _val_chunk(*args):
    """:func:`_evaluate_val_chunk`, repeated with a larger candidate buffer when the default one was too small."""
    return _chunked.with_edge_retry(lambda **kw: _evaluate_val_chunk(*args, **kw))


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
    chunk whose forward was flagged, or during which the checkpoint was switched to the fp32 kernels, is repeated on them),
    and a chunk whose candidate pairs did not fit the default buffer is repeated with a buffer sized from the reported totals.  ``h_dst_2_src`` is used as float64.
    ``tb_log`` must be None: the reference's image logging is not ported.  ``cell_size`` and ``cur_epoch``
    are unused, as in the reference.  An empty loader raises ValueError (the reference fails with a NameError)."""
    if tb_log is not None:
        raise NotImplementedError("check_val_repeatability: tensorboard image logging is not ported; pass tb_log=None")
    device = torch.device(device)
    chunk_pairs, batch_size = max(1, int(chunk_pairs)), max(1, int(batch_size))
    values, pairs = [], []

    def flush():
        args = (list(pairs), model, device, nms_size, num_points, batch_size)
        values.append(run_guarded(model, lambda: _val_chunk(*args)).values)
        pairs.clear()

    for batch in dataloader:
        images_src, images_dst, _, _, _, h_dst_2_src = batch
        pairs.append((images_src[0], images_dst[0], h_dst_2_src[0]))
        if len(pairs) == chunk_pairs:
            flush()
    if pairs:
        flush()
    if not values:
        raise ValueError("check_val_repeatability: the dataloader is empty")
    t = _chunked.Table(_REP_FIELDS, np.concatenate(values))
    # leg 0 (greedy): means over all pairs (contiguous copies: the summation order of a 1-D array); leg 1 (window): the LAST pair alone
    return tuple(np.ascontiguousarray(t[k][:, 0]).mean() for k in _MEANS) + \
        tuple(np.asarray([t[k][-1, 1]]).mean() for k in _MEANS)


def _anchor_loss_chunk(batches, model, device, grid_size, batch_size):
    """``batches``: (images_src, images_dst, heatmap_src, heatmap_dst) of some loader batches -> src_anchor_loss +
    dst_anchor_loss of each: the two float32 losses are added into a float64 device tensor, which is read once at the end
    -> float64 NumPy array, one value per batch."""
    out = torch.zeros((len(batches),), dtype=torch.float64, device=device)
    for i, (images_src, images_dst, heat_src, heat_dst) in enumerate(batches):
        for images, heat in ((images_src, heat_src), (images_dst, heat_dst)):
            images = images.to(device)
            logits = torch.cat([model(images[at:at + batch_size], want_logits=True)["logits"]
                                for at in range(0, len(images), batch_size)])
            out[i] += loss_function.detector_loss(heat.to(device).contiguous(), logits, grid_size=grid_size, device=device,
                                                  noise=False)
    return out.cpu().numpy()                                    # the one device-to-host read of the chunk


@torch.no_grad()
def check_val_anchor_loss(dataloader, model, device, grid_size=8, batch_size=16, chunk_pairs=64):
    """The quantity ``train_model`` logs as ``total_loss`` (train_utils.py:104-120), ``src_anchor_loss + dst_anchor_loss``
    (``loss_function.detector_loss`` of each side's heat map against that side's logits, no valid mask), evaluated on every
    loader batch and averaged over the batches -> a Python float.  ``dataloader`` yields the 6-tuples of
    ``check_val_repeatability``; here EVERY element of a batch counts (the loss is a mean over the batch), images are
    forwarded ``batch_size`` at a time.  ``grid_size`` must be 8 (see ``loss_function.detector_loss``).  ``noise=False``: the
    lowest channel wins a tie among the key points of a cell, so an epoch's value is reproducible (the reference's training
    step draws a random tie-break).  The per-batch sums stay on the device as float64 and are read once per ``chunk_pairs``
    batches; the mean is taken over all of them on the host, so the value does not depend on ``chunk_pairs``.  Each chunk runs
    under ``guard.run_guarded`` as the other validation loops do: a chunk whose split-f16 forward was flagged is repeated on
    the fp32 kernels.  An empty loader raises ValueError."""
    device = torch.device(device)
    chunk_pairs, batch_size = max(1, int(chunk_pairs)), max(1, int(batch_size))
    values, batches = [], []

    def flush():
        args = (list(batches), model, device, grid_size, batch_size)
        values.append(run_guarded(model, lambda: _anchor_loss_chunk(*args)))
        batches.clear()

    for batch in dataloader:
        batches.append(tuple(batch[:4]))
        if len(batches) == chunk_pairs:
            flush()
    if batches:
        flush()
    if not values:
        raise ValueError("check_val_anchor_loss: the dataloader is empty")
    return float(np.concatenate(values).mean())


def _guarded_features(model, encode_chunk):
    """``encode_chunk()`` -> its features, final with respect to the split-f16 guard: after the chunk's forwards are enqueued
    the guard is asked with a wait (``fp16_guard_check(synchronize=True)``), and the chunk is encoded again, ONCE, when that
    look finds a flag or when the checkpoint was switched to the fp32 kernels while the chunk was in flight.  The second
    condition is ``guard.run_guarded``'s: ``fp16_guard_check`` says True only when THIS look finds the flag, and a chunk is many
    forwards, each of which starts with a look at the earlier ones (and a full ring forces one) -- a flag consumed there sets
    the verdict, cannot repair a score map nobody holds any more, and leaves the flagged forward's features as they are.  The
    repeat runs on the fp32 kernels, which set no flag."""
    on_fp32 = getattr(model, "effective_precision", None) == "fp32"
    features = encode_chunk()
    flagged = model.fp16_guard_check(synchronize=True)
    if flagged or (not on_fp32 and getattr(model, "effective_precision", None) == "fp32"):
        features = encode_chunk()
    return features


def train_head(dataloader, model, head, optimizer, device, grid_size=8, chunk_batches=16, noise=None) -> float:
    """One epoch of the reference's training step (train_utils.py:104-124) for the trainable tail alone: ``model``'s encoder is
    frozen and runs on the forward kernels (``model.encode``), ``head`` (``model.head_train.TrainableHead``, or one of
    ``model.tail_train.TrainableTail``, ``model.mixer_train.TrainableMixerTail``, ``model.stage4_train.TrainableStage4`` -- all
    of stage 4 -- and ``model.stage3_train.TrainableStage3`` -- stages 3 and 4 --, whose ``encode_level`` attribute selects
    ``model.encode(x, level=...)``) runs forward in
    training mode and backward on the library, ``optimizer`` (any ``torch.optim.Optimizer`` over ``head.parameters()``; the intended
    one is ``balf_amd.optim.FusedAdam``, one launch per step, which ``build_optimizer`` returns) steps once per loader batch.
    ``dataloader`` yields the reference's 6-tuples ``(images_src, images_dst, heatmap_src, heatmap_dst, h_src_2_dst,
    h_dst_2_src)``; images ``[B,3,H,W]`` with H, W multiples of 64.  Per chunk of ``chunk_batches`` batches: every source and
    destination batch is encoded, the split-f16 guard is asked (``fp16_guard_check(synchronize=True)``), and on a flag -- found
    by that look, or consumed by a forward of the chunk itself, which shows as ``effective_precision`` having become 'fp32' --
    the chunk is encoded again, once: the checkpoint is on the fp32 kernels by then.  Only then the head steps run: ``loss =
    detector_loss(src) + detector_loss(dst)``, ``zero_grad``, ``backward``, ``step``.  The features do not depend on the head's
    updates, so the retry needs no snapshot and never repeats an optimiser step.  The per-batch losses stay on the device and
    are read once per chunk; the return value is their mean, taken on the host.  ``noise`` as in
    ``loss_function.detector_loss`` (None draws the reference's random tie-break).  ``grid_size`` must be 8; an empty loader
    raises ValueError.  ``head`` is left in training mode; ``head.commit(model)`` writes the result back."""
    if grid_size != loss_function.GRID_SIZE:
        raise ValueError(f"train_head: only grid_size={loss_function.GRID_SIZE} (the 65-channel head) is supported, got {grid_size}")
    device = torch.device(device)
    chunk_batches = max(1, int(chunk_batches))
    values, batches = [], []

    level = getattr(head, "encode_level", "x2")              # model.tail_train.TrainableTail: "rcab", features = (y, r)

    def encode(x):
        return model.encode(x) if level == "x2" else model.encode(x, level=level)

    def encode_chunk():
        return [(encode(b[0].to(device)), encode(b[1].to(device))) for b in batches]

    def flush():
        features = _guarded_features(model, encode_chunk)
        losses = torch.zeros((len(batches),), dtype=torch.float32, device=device)
        for i, (feat_src, feat_dst) in enumerate(features):
            loss = None
            for feat, heat in ((feat_src, batches[i][2]), (feat_dst, batches[i][3])):
                logits = head(feat, want_prob=False)["logits"]
                side = loss_function.detector_loss(heat.to(device).contiguous(), logits, grid_size=grid_size, device=device,
                                                   noise=noise)
                loss = side if loss is None else loss + side
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses[i] = loss.detach()
        values.append(losses.cpu().numpy())                     # the one device-to-host read of the chunk
        batches.clear()

    head.train()
    for batch in dataloader:
        batches.append(tuple(batch[:4]))
        if len(batches) == chunk_batches:
            flush()
    if batches:
        flush()
    if not values:
        raise ValueError("train_head: the dataloader is empty")
    return float(np.concatenate(values).astype(np.float64).mean())


# ---- what the reference's train.py sets a run up with (train_utils.py:20-76,199-203) ------------------------------------------------
def _all_float32_on_gpu(params) -> bool:
    """Every parameter -- of a list of tensors or of a list of group dicts -- is a dense float32 tensor on a GPU."""
    tensors = []
    for entry in params:
        tensors.extend(entry["params"] if isinstance(entry, dict) else [entry])
    return bool(tensors) and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                 and t.layout == torch.strided for t in tensors)


def build_optimizer(params, optim_cfg):
    """The reference's ``build_optimizer``: ``optim_cfg['name']`` 'adam' (``lr``, ``weight_decay``) or 'sgd' (``lr``), anything
    else a ValueError.  For float32 parameters on a GPU the optimiser is ``balf_amd.optim.FusedAdam`` / ``FusedSGD`` -- the same
    update in one launch per group, with a ``state_dict`` that torch's class loads and vice versa --, otherwise
    (parameters on the CPU, another dtype) it is torch's own class."""
    from .. import optim as fused_optim
    logging.info("build_optimizer: %s", optim_cfg['name'])
    params = list(params)
    fused = _all_float32_on_gpu(params)
    if optim_cfg['name'] == 'adam':
        cls = fused_optim.FusedAdam if fused else torch.optim.Adam
        return cls(params, lr=optim_cfg['lr'], weight_decay=optim_cfg['weight_decay'])
    if optim_cfg['name'] == 'sgd':
        cls = fused_optim.FusedSGD if fused else torch.optim.SGD
        return cls(params, lr=optim_cfg['lr'])
    raise ValueError("Optimizer [%s] not recognized." % optim_cfg['name'])


class WarmRestart(torch.optim.lr_scheduler.CosineAnnealingLR):
    """Cosine annealing from the base lr to ``eta_min`` over ``T_max`` epochs in closed form, started again from the base lr when
    the epoch counter reaches ``T_max`` (the counter returns to 0 and the period is multiplied by ``T_mult``)."""

    def __init__(self, optimizer, T_max=30, T_mult=1, eta_min=0, last_epoch=-1):
        self.T_mult = T_mult
        super().__init__(optimizer, T_max, eta_min, last_epoch)

    def get_lr(self):
        if self.last_epoch == self.T_max:
            self.last_epoch = 0
            self.T_max *= self.T_mult
        half_cos = (1 + math.cos(math.pi * self.last_epoch / self.T_max)) / 2        # 1 at a (re)start, 0 at T_max
        return [self.eta_min + (base - self.eta_min) * half_cos for base in self.base_lrs]


class LinearDecay(torch.optim.lr_scheduler.LRScheduler):
    """The base lr until ``start_epoch``, then a straight line that falls by ``(base - min_lr) / max_epoch`` per epoch."""

    def __init__(self, optimizer, max_epoch, start_epoch=0, min_lr=0, last_epoch=-1):
        self.max_epoch, self.start_epoch, self.min_lr = max_epoch, start_epoch, min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        past = self.last_epoch - self.start_epoch
        if past < 0:
            return self.base_lrs
        return [base - ((base - self.min_lr) / self.max_epoch) * past for base in self.base_lrs]


def build_scheduler(optimizer, total_epochs, last_epoch, scheduler_cfg):
    """The reference's ``build_scheduler``: ``scheduler_cfg['name']`` 'plateau' (``patience``, ``factor``, ``min_lr``), 'sgdr'
    (:class:`WarmRestart` with its defaults) or 'linear' (:class:`LinearDecay`: ``min_lr``, ``start_epoch``, resumed at
    ``last_epoch``), anything else a ValueError."""
    logging.info("build_scheduler: %s", scheduler_cfg['name'])
    name = scheduler_cfg['name']
    if name == 'plateau':
        return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', patience=scheduler_cfg['patience'],
                                                          factor=scheduler_cfg['factor'], min_lr=scheduler_cfg['min_lr'])
    if name == 'sgdr':
        return WarmRestart(optimizer)
    if name == 'linear':
        return LinearDecay(optimizer, min_lr=scheduler_cfg['min_lr'], max_epoch=total_epochs,
                           start_epoch=scheduler_cfg['start_epoch'], last_epoch=last_epoch)
    raise ValueError("Scheduler [%s] not recognized." % name)


def ckpt_state(model=None, optimizer=None, epoch=None, rep_s=0.):
    """What the reference's train.py saves per checkpoint: ``epoch``, ``model_state``, ``optimizer_state`` (None without a model /
    an optimizer) and ``repeatability``."""
    return {'epoch': epoch, 'model_state': None if model is None else model.state_dict(),
            'optimizer_state': None if optimizer is None else optimizer.state_dict(), 'repeatability': rep_s}
