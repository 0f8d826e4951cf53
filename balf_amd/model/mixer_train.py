"""``TrainableMixerTail``: stage 4's multi-axis gated-MLP layer (``down4.residual_split_head_multi_axis_gmlp_layer``: LayerNorm,
dense1, GELU, the grid and the block branch with their 64 x 64 token mixing, dense2) followed by the ``TrainableTail`` (the
channel-attention block and the head), on the features of the frozen encoder two blocks earlier
(``MLP_MA_DECODER.encode(x, level="gmlp")`` -> ``x0``); forward in training mode and backward on the HIP library
(``train_units.gmlp_step``: balf_gmlp_train_forward_c / balf_gmlp_train_backward_c, include/balf_hip.h).  The gradient that the block's backward
writes for its input (``dy``) is what this layer's backward starts from.

Like the tail, the module owns COPIES of its parameters; the model is not touched while it trains, and ``commit(model)`` writes
the 26 parameters here and the tail's tensors back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .tail_train import TrainableTail
from .train_units import _GmlpTrain, check_eps, copy_params, gmlp_step      # noqa: F401  (_GmlpTrain: tests import it from here)


_PREFIX = "down4.residual_split_head_multi_axis_gmlp_layer."


def _register(root: nn.Module, name: str, shape) -> None:
    """``root.<a>.<b>... = Parameter(zeros(shape))`` under the dotted state-dict ``name``, with plain holder modules on the way."""
    *path, leaf = name.split(".")
    m = root
    for part in path:
        if not hasattr(m, part):
            setattr(m, part, nn.Module())
        m = getattr(m, part)
    m.register_parameter(leaf, nn.Parameter(torch.zeros(shape)))


class TrainableMixerTail(nn.Module):
    encode_level = "gmlp"               # what utils.train_utils.train_head asks of model.encode for this module

    def __init__(self, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.mixer = nn.Module()        # the 26 parameters under their names inside the layer
        for name, shape in ops.gmlp_param_shapes(256).items():
            _register(self.mixer, name, shape)
        self.tail = TrainableTail(eps, momentum)

    def gmlp_parameters(self):
        """The 26 tensors of the layer in ``ops.GMLP_PARAMS`` order."""
        own = dict(self.mixer.named_parameters())
        return tuple(own[n] for n in ops.GMLP_PARAMS)

    @classmethod
    def from_model(cls, model) -> "TrainableMixerTail":
        """A module holding copies of ``model``'s gMLP layer of stage 4, of its channel-attention block and of its head (float32,
        on the model's device), in training mode."""
        check_eps("TrainableMixerTail", layer=model.down4.residual_split_head_multi_axis_gmlp_layer)
        tail = TrainableTail.from_model(model)
        mine = cls(eps=tail.head.norm.eps, momentum=tail.head.norm.momentum)
        src = model.state_dict()
        mine.to(src[_PREFIX + ops.GMLP_PARAMS[0]].device)
        mine.tail = tail
        copy_params(mine.mixer.named_parameters(), src, _PREFIX)
        return mine

    def commit(self, model) -> None:
        """Write the 26 parameters of the layer and everything of the tail back into ``model``, in place: the model's cache key
        sees the update and its next forward re-packs the weights once."""
        copy_params(self.mixer.named_parameters(), model.state_dict(), _PREFIX, back=True)
        self.tail.commit(model)

    def forward(self, x0: torch.Tensor, want_prob: bool = True):
        """``x0`` = ``model.encode(x, level="gmlp")`` -> what ``TrainableHead.forward`` returns.  ``train()`` mode: the result
        carries the graph when gradients are enabled and a parameter or ``x0`` requires one.  ``x0`` feeds the layer, the layer's
        own shortcut and the block's long shortcut ``r = y + x0``; when it requires a gradient it receives all three (the long
        shortcut's through ``r``, which is otherwise a constant).  ``eval()`` mode: the same arithmetic without a graph."""
        return self.tail(gmlp_step(x0, self.gmlp_parameters(), self.training), want_prob=want_prob)
