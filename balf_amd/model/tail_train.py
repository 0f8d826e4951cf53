"""``TrainableTail``: stage 4's channel-attention block (``down4.residual_channel_attention_block``: LayerNorm, two Linears
around a LeakyReLU, the squeeze-excite scale) followed by the ``TrainableHead`` (``down4.conv2``, ReLU, ``detector_head``), on the
features of the frozen encoder one block earlier (``MLP_MA_DECODER.encode(x, level="rcab")`` -> ``(y, r)``); forward in training
mode and backward on the HIP library (balf_rcab_train_forward / balf_rcab_train_backward, include/balf_hip.h).
The gradient that the head's backward writes for its input (``dx2``) is what this block's backward starts from.

Like the head, the tail owns COPIES of its parameters; the model is not touched while it trains, and ``commit(model)`` writes
the ten parameters here and the head's tensors back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops
from .head_train import TrainableHead


class _RcabTrain(torch.autograd.Function):
    """Forward keeps the kernel's ``saved`` block; backward is one balf_rcab_train_backward call (dy only if ``y`` requires a
    gradient).  ``r`` = y + the long shortcut is a constant of the frozen encoder for ``TrainableTail``; when it does require a
    gradient (``model.mixer_train.TrainableMixerTail`` with an input that requires one) that gradient is dx2 itself."""

    @staticmethod
    def forward(ctx, y, r, *params):
        out = ops.rcab_train_forward(y, r, params)
        ln_g, _, wc1, _, wc2, _, ws0, _, ws2, _ = params
        ctx.save_for_backward(y, ln_g, wc1, wc2, ws0, ws2, out.saved)
        return out.x2

    @staticmethod
    @once_differentiable
    def backward(ctx, dx2):
        y, ln_g, wc1, wc2, ws0, ws2, saved = ctx.saved_tensors
        g = ops.rcab_train_backward(dx2.contiguous(), y, ln_g, wc1, wc2, ws0, ws2, saved, want_dy=ctx.needs_input_grad[0])
        return (g.dy, dx2 if ctx.needs_input_grad[1] else None) + tuple(g[:10])


class _Holder(nn.Module):
    pass


_PREFIX = "down4.residual_channel_attention_block."
_NAMES = ("norm.weight", "norm.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "calayer.excite.0.weight",
          "calayer.excite.0.bias", "calayer.excite.2.weight", "calayer.excite.2.bias")       # in ops.RCAB_PARAMS order


class TrainableTail(nn.Module):
    encode_level = "rcab"               # what utils.train_utils.train_head asks of model.encode for this module

    def __init__(self, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.norm = nn.LayerNorm(256)
        self.conv1 = nn.Linear(256, 256)
        self.conv2 = nn.Linear(256, 256)
        self.calayer = _Holder()
        self.calayer.excite = nn.Sequential(nn.Linear(256, 64), nn.ReLU(inplace=True), nn.Linear(64, 256), nn.Sigmoid())
        self.head = TrainableHead(eps, momentum)

    def rcab_parameters(self):
        """The ten tensors of the block in ``ops.RCAB_PARAMS`` order."""
        own = dict(self.named_parameters())
        return tuple(own[n] for n in _NAMES)

    @classmethod
    def from_model(cls, model) -> "TrainableTail":
        """A tail holding copies of ``model``'s channel-attention block of stage 4 and of its head (float32, on the model's
        device), in training mode."""
        if model.down4.residual_channel_attention_block.norm.eps != 1e-5:
            raise ValueError("TrainableTail: the library's LayerNorm has eps = 1e-5")
        head = TrainableHead.from_model(model)
        tail = cls(eps=head.norm.eps, momentum=head.norm.momentum)
        src = model.state_dict()
        tail.to(src[_PREFIX + _NAMES[0]].device)
        tail.head = head
        with torch.no_grad():
            for n, p in zip(_NAMES, tail.rcab_parameters()):
                p.copy_(src[_PREFIX + n])
        return tail

    def commit(self, model) -> None:
        """Write the ten parameters of the block and everything of the head back into ``model``, in place: the model's cache key
        sees the update and its next forward re-packs the weights once."""
        dst = model.state_dict()
        with torch.no_grad():
            for n, p in zip(_NAMES, self.rcab_parameters()):
                dst[_PREFIX + n].copy_(p)
        self.head.commit(model)

    def forward(self, features, want_prob: bool = True):
        """``features`` = ``(y, r)`` of ``model.encode(x, level="rcab")`` -> what ``TrainableHead.forward`` returns.  ``train()``
        mode: the result carries the graph when gradients are enabled and a parameter or ``y`` requires one (``dy`` is computed
        only for ``y``).  ``eval()`` mode: the same arithmetic without a graph, and the head in eval mode."""
        y, r = features
        params = self.rcab_parameters()
        wanted = y.requires_grad or r.requires_grad or any(p.requires_grad for p in params)
        if self.training and torch.is_grad_enabled() and wanted:
            x2 = _RcabTrain.apply(y, r, *params)
        else:
            x2 = ops.rcab_train_forward(y.detach(), r.detach(), tuple(p.detach() for p in params)).x2
        return self.head(x2, want_prob=want_prob)
