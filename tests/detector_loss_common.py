"""Shared by tests/test_detector_loss_host.py, tests/test_detector_loss_gpu.py, tests/golden/make_detector_loss_golden.py and
tools/bench_loss.py: the fixture detector_loss.npz, the float64 restatement of the reference's detector_loss
(balf/loss/loss_function.py:7-26) that the GPU results are gated against, the same composition in float32 torch ops, and the
seeded case generator for shapes that have no fixture."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_loss.npz")
# name, (B, Hc, Wc), seed, logit scale, with a mask
FIXTURE_CASES = (("one", (1, 1, 1), 11, 4.0, True),
                 ("small", (3, 3, 5), 12, 4.0, True),
                 ("mid", (2, 9, 15), 13, 4.0, True),
                 ("big_logits", (1, 5, 7), 14, 100.0, True),
                 ("no_mask", (2, 8, 8), 15, 4.0, False))
TOL_FLOOR = 2.0 ** -21          # eight ulps of a float32 result


def fixture():
    return np.load(FIXTURE)


def space_to_depth(t):
    """[B,1,8Hc,8Wc] -> [B,64,Hc,Wc], channel dy * 8 + dx (tensor_op.pixel_shuffle_inv with one input channel)."""
    b, _, h, w = t.shape
    return t.reshape(b, h // 8, 8, w // 8, 8).permute(0, 2, 4, 1, 3).reshape(b, 64, h // 8, w // 8)


def make_case(shape, seed, scale=4.0, with_mask=True, density=0.03, mask_zeros=0.002, last_masked=True):
    """Seeded inputs -> dict of float32 torch tensors on the CPU: logits [B,65,Hc,Wc] (normal * scale), keypoint_map
    [B,1,8Hc,8Wc] of zeros and ones (``density`` ones, so that some cells hold several), valid_mask (``mask_zeros`` zeros; the
    last image of a batch of several fully masked) or None, noise [B,65,Hc,Wc] uniform in [0, 0.1)."""
    b, hc, wc = shape
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((b, 65, hc, wc), generator=g) * scale
    kp = (torch.rand((b, 1, 8 * hc, 8 * wc), generator=g) < density).float()
    vm = None
    if with_mask:
        vm = (torch.rand((b, 1, 8 * hc, 8 * wc), generator=g) >= mask_zeros).float()
        if b > 1 and last_masked:
            vm[-1] = 0.0
    noise = torch.rand((b, 65, hc, wc), generator=g) * 0.1
    return {"logits": logits, "keypoint_map": kp, "valid_mask": vm, "noise": noise}


def labels_f32(keypoint_map, noise):
    """The label arithmetic, float32 as the reference's: argmax of cat(2 * s2d(kp), 1) + noise, first index of the maximum."""
    b, _, h, w = keypoint_map.shape
    v = torch.cat([2 * space_to_depth(keypoint_map.float()), torch.ones((b, 1, h // 8, w // 8), device=keypoint_map.device)], dim=1)
    if noise is not None:
        v = v + noise
    return torch.argmax(v, dim=1)


def restate64(logits, keypoint_map, valid_mask=None, noise=None):
    """The float64 restatement: only the label arithmetic is float32; lse in float64, den as the float64 sum of float32 terms.
    -> dict(loss, per_image [B], labels [B,Hc,Wc] int64, grad [B,65,Hc,Wc], den [B]) of float64 / int64 NumPy arrays."""
    labels = labels_f32(keypoint_map, noise)
    b = logits.shape[0]
    vm = torch.ones_like(keypoint_map) if valid_mask is None else valid_mask
    vm = torch.prod(space_to_depth(vm.float()), dim=1)                                     # exact for zeros and ones
    z = logits.double()
    lse = torch.logsumexp(z, dim=1)
    ce = lse - torch.gather(z, 1, labels[:, None])[:, 0]
    den = (vm + torch.tensor(1e-6, dtype=torch.float32)).double().sum(dim=(1, 2))
    per_image = (ce * vm.double()).sum(dim=(1, 2)) / den
    onehot = torch.zeros_like(z).scatter_(1, labels[:, None], 1.0)
    grad = (torch.softmax(z, dim=1) - onehot) * vm.double()[:, None] / (den[:, None, None, None] * b)
    return {"loss": per_image.mean().numpy(), "per_image": per_image.numpy(), "labels": labels.numpy(), "grad": grad.numpy(),
            "den": den.numpy()}


def compose_f32(logits, keypoint_map, valid_mask=None, noise=None, want_grad=False):
    """The same quantity from float32 torch ops on the tensors' device (the noise handed in instead of drawn): labels as
    above, cell mask, log-softmax picked at the label, masked per-image mean, batch mean -> loss, or (loss, dlogits) through
    autograd."""
    if want_grad:
        logits = logits.detach().requires_grad_()
    labels = labels_f32(keypoint_map, noise)
    ce = -torch.log_softmax(logits, dim=1).gather(1, labels[:, None])[:, 0]
    cell_ok = torch.ones_like(ce) if valid_mask is None else space_to_depth(valid_mask).prod(dim=1)
    loss = ((ce * cell_ok).sum((1, 2)) / (cell_ok + 1e-6).sum((1, 2))).mean()
    if not want_grad:
        return loss
    loss.backward()
    return loss.detach(), logits.grad


def loss_error(got, want64):
    """|got - want| / max(|want|, 1), the normalisation of tol_loss."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    return float(np.max(np.abs(got - want64) / np.maximum(np.abs(want64), 1.0)))


def grad_error(got, want64, den):
    """max |got - want| * den_b * B, the normalisation of tol_grad (the gradient of a cell is (softmax - onehot) * vm over that)."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    return float(np.max(np.abs(got - want64) * (np.asarray(den, np.float64) * got.shape[0])[:, None, None, None]))
