"""``TrainableTail``: stage 4's channel-attention block (``down4.residual_channel_attention_block``: LayerNorm, two Linears
around a LeakyReLU, the squeeze-excite scale) followed by the ``TrainableHead`` (``down4.conv2``, ReLU, ``detector_head``), on the
features of the frozen encoder one block earlier (``MLP_MA_DECODER.encode(x, level="rcab")`` -> ``(y, r)``); forward in training
mode and backward on the HIP library (``train_units.rcab_step``: balf_rcab_train_forward_c / balf_rcab_train_backward_c, include/balf_hip.h).
The gradient that the head's backward writes for its input (``dx2``) is what this block's backward starts from.

Like the head, the tail owns COPIES of its parameters; the model is not touched while it trains, and ``commit(model)`` writes
the ten parameters here and the head's tensors back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch.nn as nn

from .head_train import TrainableHead
from .train_units import _RcabTrain, check_eps, copy_params, rcab_step      # noqa: F401  (_RcabTrain: tests import it from here)


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
        check_eps("TrainableTail", block=model.down4.residual_channel_attention_block)
        head = TrainableHead.from_model(model)
        tail = cls(eps=head.norm.eps, momentum=head.norm.momentum)
        src = model.state_dict()
        tail.to(src[_PREFIX + _NAMES[0]].device)
        tail.head = head
        copy_params(zip(_NAMES, tail.rcab_parameters()), src, _PREFIX)
        return tail

    def commit(self, model) -> None:
        """Write the ten parameters of the block and everything of the head back into ``model``, in place: the model's cache key
        sees the update and its next forward re-packs the weights once."""
        copy_params(zip(_NAMES, self.rcab_parameters()), model.state_dict(), _PREFIX, back=True)
        self.head.commit(model)

    def forward(self, features, want_prob: bool = True):
        """``features`` = ``(y, r)`` of ``model.encode(x, level="rcab")`` -> what ``TrainableHead.forward`` returns.  ``train()``
        mode: the result carries the graph when gradients are enabled and a parameter or ``y`` requires one (``dy`` is computed
        only for ``y``).  ``eval()`` mode: the same arithmetic without a graph, and the head in eval mode."""
        y, r = features
        return self.head(rcab_step(y, r, self.rcab_parameters(), self.training), want_prob=want_prob)
