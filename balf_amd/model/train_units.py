"""The units of a Down stage in training form, each stated once at the width its parameters state: the autograd functions over
the HIP library's forward and backward calls (balf_linrelu_train_*, balf_gmlp_train_*_c, balf_rcab_train_*_c, balf_pool_train_*,
include/balf_hip.h), the three steps of ``Down.forward`` -- ``conv.0`` and its ReLU, the multi-axis gated-MLP layer with the long
shortcut, the channel-attention block -- and the 2 x 2 max-pool, each with its train / eval branch, and what the trainable modules
share of ``from_model`` / ``commit``.  ``TrainableTail``, ``TrainableMixerTail``, ``TrainableStage4`` and ``TrainableStage3`` are
these steps on their own parameters."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import ops


def _width(params) -> int:
    """The width a unit's parameters state: the length of the first (``norm.weight`` / ``ln_g``).  Never read from the activation:
    the ops refuse an activation of another width."""
    return params[0].numel() if params else 0


class _LinreluTrain(torch.autograd.Function):
    """Forward keeps x3 and the output (the ReLU's derivative is taken from it); backward is one balf_linrelu_train_backward call
    (dx only if ``x3`` requires a gradient)."""

    @staticmethod
    def forward(ctx, x3, weight, bias):
        y = ops.linrelu_train_forward(x3, weight, bias).y
        ctx.save_for_backward(x3, weight, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x3, weight, y = ctx.saved_tensors
        out = ops.linrelu_train_backward(g.contiguous(), y, x3, weight, want_dx=ctx.needs_input_grad[0])
        return out.dx, out.dweight, out.dbias


class _GmlpTrain(torch.autograd.Function):
    """Forward keeps the kernel's ``saved`` block; backward is one balf_gmlp_train_backward_c call (dx0 only if ``x0`` requires a
    gradient)."""

    @staticmethod
    def forward(ctx, x0, *params):
        out = ops.gmlp_train_forward(x0, params, channels=_width(params))
        ctx.save_for_backward(x0, out.saved, *params)
        return out.y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x0, saved, *params = ctx.saved_tensors
        g = ops.gmlp_train_backward(dy.contiguous(), x0, params, saved, want_dx0=ctx.needs_input_grad[0], channels=_width(params))
        return (g.dx0,) + tuple(g.grads)


class _RcabTrain(torch.autograd.Function):
    """Forward keeps the kernel's ``saved`` block; backward is one balf_rcab_train_backward_c call (dy only if ``y`` requires a
    gradient).  ``r`` = y + the long shortcut is a constant of the frozen encoder for ``TrainableTail``; when it does require a
    gradient (``gmlp_step`` with an input that requires one) that gradient is dx2 itself."""

    @staticmethod
    def forward(ctx, y, r, *params):
        out = ops.rcab_train_forward(y, r, params, channels=_width(params))
        ln_g, _, wc1, _, wc2, _, ws0, _, ws2, _ = params
        ctx.save_for_backward(y, ln_g, wc1, wc2, ws0, ws2, out.saved)
        return out.x2

    @staticmethod
    @once_differentiable
    def backward(ctx, dx2):
        y, ln_g, wc1, wc2, ws0, ws2, saved = ctx.saved_tensors
        g = ops.rcab_train_backward(dx2.contiguous(), y, ln_g, wc1, wc2, ws0, ws2, saved, want_dy=ctx.needs_input_grad[0],
                                    channels=ln_g.numel())
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


# ---- the steps: the graph in train() mode when something asks for a gradient, else the same arithmetic on detached tensors ----
def wants_graph(train: bool, *tensors) -> bool:
    return train and torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _detached(tensors):
    return tuple(t.detach() for t in tensors)


def conv0_step(x, params, train: bool):
    """``conv.0`` (``ops.LINRELU_PARAMS``) and its ReLU -> x0; ``dx`` is computed only for an ``x`` that requires a gradient."""
    if wants_graph(train, x, *params):
        return _LinreluTrain.apply(x, *params)
    return ops.linrelu_train_forward(x.detach(), *_detached(params)).y


def gmlp_step(x0, params, train: bool):
    """The gated-MLP layer (``ops.GMLP_PARAMS``) -> (y, r): ``x0`` feeds the layer, the layer's own shortcut and the block's long
    shortcut ``r = y + x0``; when it requires a gradient it receives all three (the long shortcut's through ``r``, which is
    otherwise a constant)."""
    if wants_graph(train, x0, *params):
        y = _GmlpTrain.apply(x0, *params)
    else:
        y = ops.gmlp_train_forward(x0.detach(), _detached(params), channels=_width(params)).y
    r = (y + x0).detach()
    if wants_graph(train, x0):
        r = r + (x0 - x0.detach())                              # the same values (+ 0), and dx2 on its way to x0
    return y, r


def rcab_step(y, r, params, train: bool):
    """The channel-attention block (``ops.RCAB_PARAMS``) -> x2; ``dy`` is computed only for a ``y`` that requires a gradient."""
    if wants_graph(train, y, r, *params):
        return _RcabTrain.apply(y, r, *params)
    return ops.rcab_train_forward(y.detach(), r.detach(), _detached(params), channels=_width(params)).x2


def pool_step(x, train: bool):
    """The 2 x 2 max-pool that ends a Down stage."""
    if wants_graph(train, x):
        return _PoolTrain.apply(x)
    return ops.pool_train_forward(x.detach()).out


# ---- from_model / commit ------------------------------------------------------------------------------------------------------
_GMLP_NORMS = ("norm", "grid_gmlp_layer.norm", "grid_gmlp_layer.grid_gating_unit.norm", "block_gmlp_layer.norm",
               "block_gmlp_layer.block_gating_unit.norm")


def check_eps(who: str, block=None, layer=None) -> None:
    """The LayerNorms of a model's channel-attention ``block`` and / or gated-MLP ``layer`` have the library's eps."""
    norms = ([block.norm] if block is not None else []) + ([layer.get_submodule(n) for n in _GMLP_NORMS] if layer is not None else [])
    if any(n.eps != 1e-5 for n in norms):
        raise ValueError(f"{who}: the library's LayerNorm has eps = 1e-5")


def copy_params(named, state, prefix: str, back: bool = False) -> None:
    """``named``: (name, parameter) pairs of a trainable module; ``state``: a model's ``state_dict()``.  Copy each parameter in
    from ``state[prefix + name]``, or with ``back`` out into it, in place."""
    with torch.no_grad():
        for n, p in named:
            if back:
                state[prefix + n].copy_(p)
            else:
                p.copy_(state[prefix + n])
