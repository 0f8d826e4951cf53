#!/usr/bin/env python3
"""Record tests/golden/rcab_train.npz from the REFERENCE's own modules and PyTorch's autograd on the CPU.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    python tests/golden/make_rcab_train_golden.py

Case ``model``: the reference's MLP_MA_DECODER with synth.synthetic_state_dict(0) in .train() on the seeded 2 x 3 x 64 x 64 image
of tests/head_train_common.py: model_inputs.  Forward-pre-hooks capture y at down4.residual_channel_attention_block and x2 at
down4.conv2 (retain_grad both), a forward hook on down4.conv.0's ReLU gives the long shortcut x0, and the seeded dlogits goes
back with (logits * g).sum().backward().  Stored: y, r = y + x0, dx2 = x2.grad (the inputs), and the reference's float32 x2, ten
parameter gradients and y.grad.  Case ``edges``: rcab_train_common.edges_inputs through the reference's
ResidualChannelAttentionBlock class, constructed on its own.  Also stored: the distances of the pre-activations from the two
kinks, a SHA-256 of the inputs that are regenerated instead of stored, and the gates: d_T = the largest err
(rcab_train_common.err, against the float64 restatement) of the reference's own float32 result over the cases, tol_T = max(4 *
d_T, 1.1e-6).  Large results are recorded on some rows only (rcab_train_common.recorded_part).  Nothing of the reference is
committed: the fixture holds numbers only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_model                                      # noqa: E402  (puts the reference on the path)
from balf.model.mlp_ma_decoder import ResidualChannelAttentionBlock                 # noqa: E402  (reference)
from tests import rcab_train_common as R                                            # noqa: E402


def block_grads(block, y):
    own = dict(block.named_parameters())
    out = {"d" + k: own[n].grad for k, n in R.SD_NAMES.items()}
    out["dy"] = y.grad
    return out


def run_model_case():
    image, p, dlogits, _ = R.model_inputs()
    m, _ = ref_model(0)
    m.train()
    seen = {}

    def keep(name):
        def hook(_module, args):
            args[0].retain_grad()
            seen[name] = args[0]
        return hook

    handles = [m.down4.residual_channel_attention_block.register_forward_pre_hook(keep("y")),
               m.down4.conv2.register_forward_pre_hook(keep("x2")),
               m.down4.conv.register_forward_hook(lambda _m, _a, out: seen.__setitem__("x0", out.detach().clone()))]
    out = m(image)
    for h in handles:
        h.remove()
    (out["logits"] * dlogits).sum().backward()
    y = seen["y"]
    got = dict(block_grads(m.down4.residual_channel_attention_block, y), x2=seen["x2"].detach())
    return y.detach().contiguous(), (y.detach() + seen["x0"]).contiguous(), p, seen["x2"].grad.contiguous(), got


def run_edges_case():
    y, r, p, g = R.edges_inputs()
    block = ResidualChannelAttentionBlock(256).train()
    own = dict(block.named_parameters())
    with torch.no_grad():
        for k, n in R.SD_NAMES.items():
            own[n].copy_(p[k])
    yy = y.clone().requires_grad_()
    x2 = block(yy) + (r - y)                                   # the block adds its own shortcut y; r - y is the long one
    x2.backward(g)
    return y, r, p, g, dict(block_grads(block, yy), x2=x2.detach())


def main():
    torch.manual_seed(0)
    fx = {"meta.names": np.asarray(R.FIXTURE_CASES)}
    d = {k: 0.0 for k in R.GATED}
    for name, run in (("model", run_model_case), ("edges", run_edges_case)):
        y, r, p, g, got = run()
        res = R.restate64(y, r, p, g)
        ag = R.autograd64(y, r, p, g)
        for k in R.GRADS:
            assert R.err(ag[k], res[k], res["S"][k]) <= 1e-12, (name, k)
        kink = R.kink_distances(res)
        assert min(kink) >= R.KINK_MARGIN, (name, kink)
        line = []
        for k in R.GATED:
            e = R.err(got[k], res[k], res["S"][k])
            d[k] = max(d[k], e)
            line.append(f"{k} {e:.2e}")
            fx[f"{name}.{k}"] = R.recorded_part(got[k].detach()).numpy().astype(np.float32)
        print(f"{name:6s} N {y.numel() // 256} kink lrelu {kink[0]:.2e} se {kink[1]:.2e} " + " ".join(line))
        fx[f"{name}.kink"] = np.asarray(kink, np.float64)
        fx[f"{name}.inputs_sha256"] = np.asarray(R.regenerated_inputs_digest(name))
        if name == "model":
            fx["model.y"], fx["model.r"], fx["model.dx2"] = y.numpy(), r.numpy(), g.numpy()
        else:
            h = res["h"].reshape(*R.EDGES_SHAPE, 256)[R.EDGES_CONST_ROW]
            assert bool((h[:R.EDGES_H0] == 0).all()) and bool((res["xhat"].reshape(*R.EDGES_SHAPE, 256)[R.EDGES_CONST_ROW] == 0).all())
            assert bool((res["se_pre"][:, R.EDGES_E0] == 0).all())
    for k in R.GATED:
        fx[f"d_{k}"], fx[f"tol_{k}"] = np.float64(d[k]), np.float64(max(4 * d[k], R.TOL_FLOOR))
        print(f"d_{k} {d[k]:.3e} tol {max(4 * d[k], R.TOL_FLOOR):.3e}")
    np.savez_compressed(R.FIXTURE, **fx)
    print("wrote", R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes")
    assert os.path.getsize(R.FIXTURE) < 1000000


if __name__ == "__main__":
    main()
