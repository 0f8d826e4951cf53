"""``detector_loss`` of /root/reference/balf/loss/loss_function.py:7-26 on the GPU: the labels, the masked cross-entropy and,
when the logits require it, the gradient with respect to them, all from one pass of ``balf_detector_loss``
(include/balf_hip.h; ``ops.detector_loss``).  The network's backward, optimisers and ``train_model`` are not part of this
library: a model whose backward PyTorch runs can train against this loss."""
from __future__ import annotations

import torch

from .. import ops

GRID_SIZE = 8          # the cell size of the 65-channel head, the only one arch.py supports


class _DetectorLoss(torch.autograd.Function):
    """Forward asks for dlogits in the same call; backward is the one torch multiply grad_output * dlogits."""

    @staticmethod
    def forward(ctx, logits, keypoint_map, valid_mask, noise):
        out = ops.detector_loss(logits, keypoint_map, valid_mask, noise, want_grad=True)
        ctx.save_for_backward(out.dlogits)
        return out.loss

    @staticmethod
    def backward(ctx, grad_output):
        (dlogits,) = ctx.saved_tensors
        return grad_output * dlogits, None, None, None


def detector_loss(keypoint_map, logits, valid_mask=None, grid_size=8, device=None, noise=None):
    """The reference's signature and argument order -> the 0-dim float32 loss on the GPU.

    ``keypoint_map`` [B,1,H,W] (any dtype: it goes through ``.float()`` as in the reference), ``logits`` [B,65,H/8,W/8]
    float32, ``valid_mask`` [B,1,H,W] float32 or None (all ones).  ``grid_size`` must be 8 (the reference's ``train_model``
    passes 16, which its own 65-channel head cannot satisfy).  ``device`` is accepted for the reference's call sites and must
    name the tensors' device.  ``noise``: None draws the reference's random tie-break,
    ``torch.empty(B,65,Hc,Wc).uniform_(0, 0.1)`` from torch's generator (torch supplies the random numbers, not the
    arithmetic); False uses none (the lowest channel wins a tie, reproducibly); a [B,65,Hc,Wc] float32 tensor is used as it
    is.  When ``logits.requires_grad`` (and gradients are enabled) the result carries the gradient; otherwise none is computed."""
    if grid_size != GRID_SIZE:
        raise ValueError(f"detector_loss: only grid_size={GRID_SIZE} (the 65-channel head) is supported, got {grid_size}")
    if keypoint_map.dim() != 4 or keypoint_map.shape[1] != 1 or logits.dim() != 4:
        raise ValueError(f"detector_loss: keypoint_map must be [B,1,H,W] and logits [B,65,H/8,W/8], got "
                         f"{tuple(keypoint_map.shape)} and {tuple(logits.shape)}")
    b, _, h, w = keypoint_map.shape
    if h % GRID_SIZE or w % GRID_SIZE or tuple(logits.shape) != (b, 65, h // GRID_SIZE, w // GRID_SIZE):
        raise ValueError(f"detector_loss: logits must be [B,65,H/8,W/8] = {[b, 65, h // GRID_SIZE, w // GRID_SIZE]} for a "
                         f"keypoint_map of {list(keypoint_map.shape)} (grid_size 8, 65 channels), got {list(logits.shape)}")
    if device is not None:
        d = torch.device(device)
        if d.type != logits.device.type or (d.index is not None and d.index != logits.device.index):
            raise ValueError(f"detector_loss: device={device!r} but the logits are on {logits.device}")
    if noise is None:
        noise = torch.empty((b, 65, h // GRID_SIZE, w // GRID_SIZE), device=logits.device).uniform_(0, 0.1)
    elif noise is False:
        noise = None
    keypoint_map = keypoint_map.float()
    if logits.requires_grad and torch.is_grad_enabled():
        return _DetectorLoss.apply(logits, keypoint_map, valid_mask, noise)
    return ops.detector_loss(logits.detach(), keypoint_map, valid_mask, noise).loss
