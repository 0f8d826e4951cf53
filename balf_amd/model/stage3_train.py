"""``TrainableStage3``: all of stage 3 -- ``down3.conv.0`` (Linear 64 -> 128) and its ReLU, the multi-axis gated-MLP layer and
the channel-attention block at 128 channels, the long shortcut and the 2 x 2 max-pool -- followed by the ``TrainableStage4``
(all of stage 4 and the head), on the output of the frozen stages 1-2 (``MLP_MA_DECODER.encode(x, level="stage2")`` ->
``x2s``); forward in training mode and backward on the HIP library (the steps of ``train_units`` at C = 128: balf_linrelu_train_*,
balf_gmlp_train_*_c, balf_rcab_train_*_c, balf_pool_train_*, include/balf_hip.h).  The counterpart of the reference's
``Down.forward`` of ``down3``.  As in stage 4, the output ``x0`` of ``conv.0`` feeds the gated-MLP layer, that layer's shortcut and
the block's long shortcut ``r = y + x0``; autograd adds the three gradients, and the sum is what ``conv.0``'s backward starts from.

Like the modules below it, this one owns COPIES of its parameters (38 tensors of ``down3.*``; 82 with stage 4 and the head); the
model is not touched while it trains, and ``commit(model)`` writes everything back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .mixer_train import _register
from .stage4_train import TrainableStage4
from .tail_train import _NAMES as _RCAB_NAMES
from .train_units import _PoolTrain, check_eps, conv0_step, copy_params, gmlp_step, pool_step, rcab_step    # noqa: F401  (_PoolTrain)

CHANNELS = 128
_CONV0 = "conv.0."
_GMLP = "residual_split_head_multi_axis_gmlp_layer."
_RCAB = "residual_channel_attention_block."
_PREFIX = "down3."


class TrainableStage3(nn.Module):
    encode_level = "stage2"             # what utils.train_utils.train_head asks of model.encode for this module

    def __init__(self, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.down3 = nn.Module()        # the 38 tensors under their names inside down3
        _register(self.down3, _CONV0 + "weight", (CHANNELS, CHANNELS // 2))
        _register(self.down3, _CONV0 + "bias", (CHANNELS,))
        for name, shape in ops.gmlp_param_shapes(CHANNELS).items():
            _register(self.down3, _GMLP + name, shape)
        for name, shape in zip(_RCAB_NAMES, ops.rcab_param_shapes(CHANNELS).values()):
            _register(self.down3, _RCAB + name, shape)
        self.stage4 = TrainableStage4(eps, momentum)

    def _named(self, prefix, names):
        own = dict(self.down3.named_parameters())
        return tuple(own[prefix + n] for n in names)

    def conv0_parameters(self):
        """The two tensors of ``down3.conv.0`` in ``ops.LINRELU_PARAMS`` order."""
        return self._named(_CONV0, ops.LINRELU_PARAMS)

    def gmlp_parameters(self):
        """The 26 tensors of stage 3's gated-MLP layer in ``ops.GMLP_PARAMS`` order."""
        return self._named(_GMLP, ops.GMLP_PARAMS)

    def rcab_parameters(self):
        """The ten tensors of stage 3's channel-attention block in ``ops.RCAB_PARAMS`` order."""
        return self._named(_RCAB, _RCAB_NAMES)

    def stage3_names(self):
        """The 38 names of this module's own tensors inside ``down3``, in the order of ``parameters()``."""
        return tuple(n for n, _ in self.down3.named_parameters())

    @classmethod
    def from_model(cls, model) -> "TrainableStage3":
        """A module holding copies of ``model``'s ``down3`` (without its unused ``conv2``) and of everything of stage 4 and the
        head below it (float32, on the model's device), in training mode."""
        check_eps("TrainableStage3", block=model.down3.residual_channel_attention_block,
                  layer=model.down3.residual_split_head_multi_axis_gmlp_layer)
        stage4 = TrainableStage4.from_model(model)
        head = stage4.mixer.tail.head
        mine = cls(eps=head.norm.eps, momentum=head.norm.momentum)
        src = model.state_dict()
        mine.to(src[_PREFIX + _CONV0 + "weight"].device)
        mine.stage4 = stage4
        copy_params(mine.down3.named_parameters(), src, _PREFIX)
        return mine

    def commit(self, model) -> None:
        """Write the 38 tensors of ``down3`` and everything of stage 4 and the head back into ``model``, in place: the model's
        cache key sees the update and its next forward re-packs the weights once."""
        copy_params(self.down3.named_parameters(), model.state_dict(), _PREFIX, back=True)
        self.stage4.commit(model)

    def forward(self, x2s: torch.Tensor, want_prob: bool = True):
        """``x2s`` = ``model.encode(x, level="stage2")`` -> what ``TrainableHead.forward`` returns.  ``train()`` mode: the result
        carries the graph when gradients are enabled and a parameter or ``x2s`` requires a gradient (``dx`` of ``conv.0`` is
        computed only for ``x2s``).  ``eval()`` mode: the same arithmetic without a graph."""
        x0 = conv0_step(x2s, self.conv0_parameters(), self.training)
        y, r = gmlp_step(x0, self.gmlp_parameters(), self.training)
        x3 = pool_step(rcab_step(y, r, self.rcab_parameters(), self.training), self.training)
        return self.stage4(x3, want_prob=want_prob)
