"""``TrainableStage4``: all of stage 4 -- ``down4.conv.0`` (Linear 128 -> 256) and its ReLU, then the ``TrainableMixerTail`` (the
multi-axis gated-MLP layer, the channel-attention block and the head) -- on the output of the frozen stages 1-3
(``MLP_MA_DECODER.encode(x, level="stage3")`` -> ``x3``); forward in training mode and backward on the HIP library
(``train_units.conv0_step``: balf_linrelu_train_forward / balf_linrelu_train_backward, include/balf_hip.h).  The output ``x0`` of this layer
feeds the gated-MLP layer, that layer's shortcut and the block's long shortcut; ``TrainableMixerTail`` hands all three gradients to
an ``x0`` that requires one, autograd adds them, and the sum is what this layer's backward starts from.

Like the blocks below it, the module owns COPIES of its parameters; the model is not touched while it trains, and
``commit(model)`` writes the two tensors here and everything below back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .mixer_train import TrainableMixerTail
from .train_units import _LinreluTrain, conv0_step, copy_params             # noqa: F401  (_LinreluTrain: tests import it from here)


_PREFIX = "down4.conv.0."


class TrainableStage4(nn.Module):
    encode_level = "stage3"             # what utils.train_utils.train_head asks of model.encode for this module

    def __init__(self, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.conv0 = nn.Module()        # down4.conv.0 under its own names, ops.LINRELU_PARAMS
        self.conv0.register_parameter("weight", nn.Parameter(torch.zeros(256, 128)))
        self.conv0.register_parameter("bias", nn.Parameter(torch.zeros(256)))
        self.mixer = TrainableMixerTail(eps, momentum)

    def conv0_parameters(self):
        """The two tensors of ``down4.conv.0`` in ``ops.LINRELU_PARAMS`` order."""
        return tuple(getattr(self.conv0, n) for n in ops.LINRELU_PARAMS)

    @classmethod
    def from_model(cls, model) -> "TrainableStage4":
        """A module holding copies of ``model``'s ``down4.conv.0`` and of everything of stage 4 and the head below it (float32, on
        the model's device), in training mode."""
        mixer = TrainableMixerTail.from_model(model)
        mine = cls(eps=mixer.tail.head.norm.eps, momentum=mixer.tail.head.norm.momentum)
        src = model.state_dict()
        mine.to(src[_PREFIX + "weight"].device)
        mine.mixer = mixer
        copy_params(mine.conv0.named_parameters(), src, _PREFIX)
        return mine

    def commit(self, model) -> None:
        """Write ``down4.conv.0`` and everything of the mixer and the tail back into ``model``, in place: the model's cache key sees
        the update and its next forward re-packs the weights once."""
        copy_params(self.conv0.named_parameters(), model.state_dict(), _PREFIX, back=True)
        self.mixer.commit(model)

    def forward(self, x3: torch.Tensor, want_prob: bool = True):
        """``x3`` = ``model.encode(x, level="stage3")`` -> what ``TrainableHead.forward`` returns.  ``train()`` mode: the result
        carries the graph when gradients are enabled and a parameter or ``x3`` requires a gradient (``dx`` is computed only for
        ``x3``).  ``eval()`` mode: the same arithmetic without a graph."""
        return self.mixer(conv0_step(x3, self.conv0_parameters(), self.training), want_prob=want_prob)
