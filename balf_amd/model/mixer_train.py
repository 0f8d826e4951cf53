"""``TrainableMixerTail``: stage 4's multi-axis gated-MLP layer (``down4.residual_split_head_multi_axis_gmlp_layer``: LayerNorm,
dense1, GELU, the grid and the block branch with their 64 x 64 token mixing, dense2) followed by the ``TrainableTail`` (the
channel-attention block and the head), on the features of the frozen encoder two blocks earlier
(``MLP_MA_DECODER.encode(x, level="gmlp")`` -> ``x0``); forward in training mode and backward on the HIP library
(balf_gmlp_train_forward / balf_gmlp_train_backward, include/balf_hip.h).  The gradient that the block's backward
writes for its input (``dy``) is what this layer's backward starts from.

Like the tail, the module owns COPIES of its parameters; the model is not touched while it trains, and ``commit(model)`` writes
the 26 parameters here and the tail's tensors back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops
from .tail_train import TrainableTail


class _GmlpTrain(torch.autograd.Function):
    """Forward keeps the kernel's ``saved`` block; backward is one balf_gmlp_train_backward call (dx0 only if ``x0`` requires a
    gradient)."""

    @staticmethod
    def forward(ctx, x0, *params):
        out = ops.gmlp_train_forward(x0, params)
        ctx.save_for_backward(x0, out.saved, *params)
        return out.y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x0, saved, *params = ctx.saved_tensors
        g = ops.gmlp_train_backward(dy.contiguous(), x0, params, saved, want_dx0=ctx.needs_input_grad[0])
        return (g.dx0,) + tuple(g.grads)


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
        for name in ops.GMLP_PARAMS:
            _register(self.mixer, name, ops._GMLP_PARAM_SHAPES[name])
        self.tail = TrainableTail(eps, momentum)

    def gmlp_parameters(self):
        """The 26 tensors of the layer in ``ops.GMLP_PARAMS`` order."""
        own = dict(self.mixer.named_parameters())
        return tuple(own[n] for n in ops.GMLP_PARAMS)

    @classmethod
    def from_model(cls, model) -> "TrainableMixerTail":
        """A module holding copies of ``model``'s gMLP layer of stage 4, of its channel-attention block and of its head (float32,
        on the model's device), in training mode."""
        layer = model.down4.residual_split_head_multi_axis_gmlp_layer
        norms = (layer.norm, layer.grid_gmlp_layer.norm, layer.grid_gmlp_layer.grid_gating_unit.norm, layer.block_gmlp_layer.norm,
                 layer.block_gmlp_layer.block_gating_unit.norm)
        if any(n.eps != 1e-5 for n in norms):
            raise ValueError("TrainableMixerTail: the library's LayerNorm has eps = 1e-5")
        tail = TrainableTail.from_model(model)
        mine = cls(eps=tail.head.norm.eps, momentum=tail.head.norm.momentum)
        src = model.state_dict()
        mine.to(src[_PREFIX + ops.GMLP_PARAMS[0]].device)
        mine.tail = tail
        with torch.no_grad():
            for n, p in zip(ops.GMLP_PARAMS, mine.gmlp_parameters()):
                p.copy_(src[_PREFIX + n])
        return mine

    def commit(self, model) -> None:
        """Write the 26 parameters of the layer and everything of the tail back into ``model``, in place: the model's cache key
        sees the update and its next forward re-packs the weights once."""
        dst = model.state_dict()
        with torch.no_grad():
            for n, p in zip(ops.GMLP_PARAMS, self.gmlp_parameters()):
                dst[_PREFIX + n].copy_(p)
        self.tail.commit(model)

    def forward(self, x0: torch.Tensor, want_prob: bool = True):
        """``x0`` = ``model.encode(x, level="gmlp")`` -> what ``TrainableHead.forward`` returns.  ``train()`` mode: the result
        carries the graph when gradients are enabled and a parameter or ``x0`` requires one.  ``x0`` feeds the layer, the layer's
        own shortcut and the block's long shortcut ``r = y + x0``; when it requires a gradient it receives all three (the long
        shortcut's through ``r``, which is otherwise a constant).  ``eval()`` mode: the same arithmetic without a graph."""
        params = self.gmlp_parameters()
        if self.training and torch.is_grad_enabled() and (x0.requires_grad or any(p.requires_grad for p in params)):
            y = _GmlpTrain.apply(x0, *params)
        else:
            y = ops.gmlp_train_forward(x0.detach(), tuple(p.detach() for p in params)).y
        r = (y + x0).detach()
        if self.training and torch.is_grad_enabled() and x0.requires_grad:
            r = r + (x0 - x0.detach())                          # the same values (+ 0), and dx2 on its way to x0
        return self.tail((y, r), want_prob=want_prob)
