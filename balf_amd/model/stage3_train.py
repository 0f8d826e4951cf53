"""``TrainableStage3``: all of stage 3 -- ``down3.conv.0`` (Linear 64 -> 128) and its ReLU, the multi-axis gated-MLP layer and
the channel-attention block at 128 channels, the long shortcut and the 2 x 2 max-pool -- followed by the ``TrainableStage4``
(all of stage 4 and the head), on the output of the frozen stages 1-2 (``MLP_MA_DECODER.encode(x, level="stage2")`` ->
``x2s``); forward in training mode and backward on the HIP library (balf_linrelu_train_*, balf_gmlp_train_*_c and
balf_rcab_train_*_c at C = 128, balf_pool_train_*, include/balf_hip.h).  The counterpart of the reference's
``Down.forward`` of ``down3``.  As in stage 4, the output ``x0`` of ``conv.0`` feeds the gated-MLP layer, that layer's shortcut and
the block's long shortcut ``r = y + x0``; autograd adds the three gradients, and the sum is what ``conv.0``'s backward starts from.

Like the modules below it, this one owns COPIES of its parameters (38 tensors of ``down3.*``; 82 with stage 4 and the head); the
model is not touched while it trains, and ``commit(model)`` writes everything back in one go, which costs the model one re-pack."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops
from .mixer_train import _register
from .stage4_train import TrainableStage4, _LinreluTrain
from .tail_train import _NAMES as _RCAB_NAMES

CHANNELS = 128
_CONV0 = "conv.0."
_GMLP = "residual_split_head_multi_axis_gmlp_layer."
_RCAB = "residual_channel_attention_block."
_PREFIX = "down3."


class _GmlpTrain128(torch.autograd.Function):
    """``mixer_train._GmlpTrain`` at 128 channels."""

    @staticmethod
    def forward(ctx, x0, *params):
        out = ops.gmlp_train_forward(x0, params, channels=CHANNELS)
        ctx.save_for_backward(x0, out.saved, *params)
        return out.y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x0, saved, *params = ctx.saved_tensors
        g = ops.gmlp_train_backward(dy.contiguous(), x0, params, saved, want_dx0=ctx.needs_input_grad[0], channels=CHANNELS)
        return (g.dx0,) + tuple(g.grads)


class _RcabTrain128(torch.autograd.Function):
    """``tail_train._RcabTrain`` at 128 channels: the gradient of ``r`` = y + the long shortcut is dx2 itself."""

    @staticmethod
    def forward(ctx, y, r, *params):
        out = ops.rcab_train_forward(y, r, params, channels=CHANNELS)
        ln_g, _, wc1, _, wc2, _, ws0, _, ws2, _ = params
        ctx.save_for_backward(y, ln_g, wc1, wc2, ws0, ws2, out.saved)
        return out.x2

    @staticmethod
    @once_differentiable
    def backward(ctx, dx2):
        y, ln_g, wc1, wc2, ws0, ws2, saved = ctx.saved_tensors
        g = ops.rcab_train_backward(dx2.contiguous(), y, ln_g, wc1, wc2, ws0, ws2, saved, want_dy=ctx.needs_input_grad[0],
                                    channels=CHANNELS)
        return (g.dy, dx2 if ctx.needs_input_grad[1] else None) + tuple(g[:10])


class _PoolTrain(torch.autograd.Function):
    """Forward keeps ``which``; backward is one balf_pool_train_backward call, which writes every element of dx."""

    @staticmethod
    def forward(ctx, x):
        out = ops.pool_train_forward(x)
        ctx.save_for_backward(out.which)
        return out.out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        which, = ctx.saved_tensors
        return ops.pool_train_backward(g.contiguous(), which)


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
        layer, block = model.down3.residual_split_head_multi_axis_gmlp_layer, model.down3.residual_channel_attention_block
        norms = (block.norm, layer.norm, layer.grid_gmlp_layer.norm, layer.grid_gmlp_layer.grid_gating_unit.norm,
                 layer.block_gmlp_layer.norm, layer.block_gmlp_layer.block_gating_unit.norm)
        if any(n.eps != 1e-5 for n in norms):
            raise ValueError("TrainableStage3: the library's LayerNorm has eps = 1e-5")
        stage4 = TrainableStage4.from_model(model)
        head = stage4.mixer.tail.head
        mine = cls(eps=head.norm.eps, momentum=head.norm.momentum)
        src = model.state_dict()
        mine.to(src[_PREFIX + _CONV0 + "weight"].device)
        mine.stage4 = stage4
        with torch.no_grad():
            for n, p in mine.down3.named_parameters():
                p.copy_(src[_PREFIX + n])
        return mine

    def commit(self, model) -> None:
        """Write the 38 tensors of ``down3`` and everything of stage 4 and the head back into ``model``, in place: the model's
        cache key sees the update and its next forward re-packs the weights once."""
        dst = model.state_dict()
        with torch.no_grad():
            for n, p in self.down3.named_parameters():
                dst[_PREFIX + n].copy_(p)
        self.stage4.commit(model)

    def forward(self, x2s: torch.Tensor, want_prob: bool = True):
        """``x2s`` = ``model.encode(x, level="stage2")`` -> what ``TrainableHead.forward`` returns.  ``train()`` mode: the result
        carries the graph when gradients are enabled and a parameter or ``x2s`` requires a gradient (``dx`` of ``conv.0`` is
        computed only for ``x2s``).  ``eval()`` mode: the same arithmetic without a graph."""
        conv0, gmlp, rcab = self.conv0_parameters(), self.gmlp_parameters(), self.rcab_parameters()
        own = conv0 + gmlp + rcab
        if self.training and torch.is_grad_enabled() and (x2s.requires_grad or any(p.requires_grad for p in own)):
            x0 = _LinreluTrain.apply(x2s, *conv0)
            y = _GmlpTrain128.apply(x0, *gmlp)
            r = (y + x0).detach()
            if x0.requires_grad:
                r = r + (x0 - x0.detach())                      # the same values (+ 0), and dx2 on its way to x0
            x3 = _PoolTrain.apply(_RcabTrain128.apply(y, r, *rcab))
        else:
            x0 = ops.linrelu_train_forward(x2s.detach(), *(p.detach() for p in conv0)).y
            y = ops.gmlp_train_forward(x0, tuple(p.detach() for p in gmlp), channels=CHANNELS).y
            x3 = ops.pool_train_forward(ops.rcab_train_forward(y, y + x0, tuple(p.detach() for p in rcab), channels=CHANNELS).x2).out
        return self.stage4(x3, want_prob=want_prob)
