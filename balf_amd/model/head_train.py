"""``TrainableHead``: the trainable tail of the detector -- ``down4.conv2`` (Linear 256 -> 256), ReLU, ``detector_head.dense``
(Linear 256 -> 65) and ``detector_head.norm`` (BatchNorm2d) -- on the features of the frozen encoder
(``MLP_MA_DECODER.encode``), forward in training mode and backward on the HIP library (balf_head_train_forward /
balf_head_train_backward, include/balf_hip.h).

The head owns COPIES of the six parameters and the three BatchNorm buffers.  The model's own tensors are not touched while the
head trains, so the model's packed blob and its split-f16 verdict stay valid and a training step costs no re-pack and no probe
forwards; ``commit(model)`` writes everything back in one go."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import ops


class _HeadTrain(torch.autograd.Function):
    """Forward keeps the kernel's ``saved`` block; backward is one balf_head_train_backward call (dx2 only if the features
    require a gradient).  No torch arithmetic on either side."""

    @staticmethod
    def forward(ctx, features, w2, b2, wd, bd, gamma, beta, running_mean, running_var, eps, momentum, want_prob):
        out = ops.head_train_forward(features, w2, b2, wd, bd, gamma, beta, eps=eps, want_prob=want_prob,
                                     running_mean=running_mean, running_var=running_var, momentum=momentum)
        ctx.save_for_backward(features, w2, wd, gamma, out.saved)
        if out.prob is None:
            return out.logits, None
        ctx.mark_non_differentiable(out.prob)
        return out.logits, out.prob

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits, _dprob):
        features, w2, wd, gamma, saved = ctx.saved_tensors
        g = ops.head_train_backward(dlogits.contiguous(), features, w2, wd, gamma, saved, want_dx2=ctx.needs_input_grad[0])
        return g.dx2, g.dw2, g.db2, g.dwd, g.dbd, g.dgamma, g.dbeta, None, None, None, None, None


class _Norm(nn.Module):
    """The parameters and buffers of a BatchNorm2d(65) under its state-dict names; the arithmetic is the library's."""

    def __init__(self, eps=1e-5, momentum=0.1):
        super().__init__()
        self.eps, self.momentum = eps, momentum
        self.weight = nn.Parameter(torch.ones(65))
        self.bias = nn.Parameter(torch.zeros(65))
        self.register_buffer("running_mean", torch.zeros(65))
        self.register_buffer("running_var", torch.ones(65))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


_PAIRS = (("conv2.weight", "down4.conv2.weight"), ("conv2.bias", "down4.conv2.bias"),
          ("dense.weight", "detector_head.dense.weight"), ("dense.bias", "detector_head.dense.bias"),
          ("norm.weight", "detector_head.norm.weight"), ("norm.bias", "detector_head.norm.bias"),
          ("norm.running_mean", "detector_head.norm.running_mean"), ("norm.running_var", "detector_head.norm.running_var"),
          ("norm.num_batches_tracked", "detector_head.norm.num_batches_tracked"))


class TrainableHead(nn.Module):
    def __init__(self, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.conv2 = nn.Linear(256, 256)
        self.dense = nn.Linear(256, 65)
        self.norm = _Norm(eps, momentum)

    @classmethod
    def from_model(cls, model) -> "TrainableHead":
        """A head holding copies of ``model``'s tail (float32, on the model's device), in training mode."""
        bn = model.detector_head.norm
        if bn.momentum is None:
            raise ValueError("TrainableHead: BatchNorm with momentum=None (cumulative average) is not supported")
        head = cls(eps=bn.eps, momentum=bn.momentum)
        src = model.state_dict()
        head.to(src["down4.conv2.weight"].device)
        with torch.no_grad():
            for mine, theirs in _PAIRS:
                head.state_dict()[mine].copy_(src[theirs])
        return head

    def commit(self, model) -> None:
        """Write the six parameters and the three BatchNorm buffers back into ``model``, in place: the model's cache key sees
        the update and its next forward re-packs the weights once."""
        dst = model.state_dict()
        mine = self.state_dict()
        with torch.no_grad():
            for name, theirs in _PAIRS:
                dst[theirs].copy_(mine[name])

    def forward(self, features: torch.Tensor, want_prob: bool = True):
        """``features`` [B,Hc,Wc,256] float32 NHWC (``model.encode``) -> {'logits' [B,65,Hc,Wc], 'prob' [B,8Hc,8Wc] or None}.
        ``train()`` mode: batch statistics, the running statistics updated by the kernel, ``num_batches_tracked`` incremented;
        the result carries the graph when gradients are enabled and a parameter or the features require one.  ``eval()`` mode:
        the running statistics, no graph."""
        n = self.norm
        params = (self.conv2.weight, self.conv2.bias, self.dense.weight, self.dense.bias, n.weight, n.bias)
        if not self.training:
            stats = torch.stack([n.running_mean, n.running_var])
            out = ops.head_train_forward(features.detach(), *(p.detach() for p in params), eps=n.eps, stats=stats,
                                         want_prob=want_prob)
            return {"logits": out.logits, "prob": out.prob}
        if torch.is_grad_enabled() and (features.requires_grad or any(p.requires_grad for p in params)):
            logits, prob = _HeadTrain.apply(features, *params, n.running_mean, n.running_var, n.eps, n.momentum, want_prob)
        else:
            out = ops.head_train_forward(features.detach(), *(p.detach() for p in params), eps=n.eps, want_prob=want_prob,
                                         running_mean=n.running_mean, running_var=n.running_var, momentum=n.momentum)
            logits, prob = out.logits, out.prob
        n.num_batches_tracked += 1
        return {"logits": logits, "prob": prob}
