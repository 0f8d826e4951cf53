#!/usr/bin/env python3
"""Record tests/golden/linrelu_train.npz from the REFERENCE's own modules and PyTorch's autograd on the CPU.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    python tests/golden/make_linrelu_train_golden.py

Case ``model``: the reference's MLP_MA_DECODER with synth.synthetic_state_dict(0) in .train() on the seeded 2 x 3 x 64 x 64 image
of tests/head_train_common.py: model_inputs.  Forward-pre-hooks capture x3 at down4.conv and x0 at
down4.residual_split_head_multi_axis_gmlp_layer (retain_grad both), and the reference's own detector_loss on the seeded labels of
linrelu_train_common.keypoint_map goes back with loss.backward().  Stored: x3 and g = x0.grad, which holds all three paths into x0
(the inputs), dlogits = logits.grad (what the GPU test sends back through TrainableStage4), and the reference's float32 x0, the two
gradients of down4.conv.0 and x3.grad.  Case ``edges``: linrelu_train_common.edges_inputs through nn.Linear(128, 256) and
nn.ReLU, constructed on their own; cases ``c32`` and ``c64``: width_inputs through nn.Linear(c_in, 2 c_in) and nn.ReLU.  Also
stored: a SHA-256 of the inputs that are regenerated instead of stored, the distance of each case from the ReLU kink, and the
gates: d_T = the largest err (linrelu_train_common.err, against the float64 restatement) of the reference's own float32 result over
the cases, tol_T = max(4 * d_T, 1.1e-6).  Nothing of the reference is committed: the fixture holds numbers only.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_functions, ref_model                       # noqa: E402  (puts the reference on the path)
from tests import linrelu_train_common as Lc                                        # noqa: E402

REF = "/root/reference/balf/"


def reference_loss():
    top = ref_functions(REF + "utils/tensor_op.py", ["pixel_shuffle_inv"], {"torch": torch})
    ns = {"torch": torch, "F": F, "tensor_op": types.SimpleNamespace(pixel_shuffle_inv=top["pixel_shuffle_inv"])}
    return ref_functions(REF + "loss/loss_function.py", ["detector_loss"], ns)["detector_loss"]


def run_model_case():
    image, (w, b), heat = Lc.model_inputs()
    m, _ = ref_model(0)
    m.train()
    seen = {}

    def keep(name):
        def hook(_module, args):
            args[0].retain_grad()
            seen[name] = args[0]
        return hook

    handles = [m.down4.conv.register_forward_pre_hook(keep("x3")),
               m.down4.residual_split_head_multi_axis_gmlp_layer.register_forward_pre_hook(keep("x0"))]
    out = m(image)
    for h in handles:
        h.remove()
    logits = out["logits"]
    logits.retain_grad()
    torch.manual_seed(0)                                        # the tie-break noise, which these labels leave without effect
    reference_loss()(heat, logits).backward()
    x3, x0 = seen["x3"], seen["x0"]
    conv0 = m.down4.conv[0]
    assert torch.equal(conv0.weight.detach(), w) and torch.equal(conv0.bias.detach(), b)
    got = {"y": x0.detach(), "dw": conv0.weight.grad, "db": conv0.bias.grad, "dx": x3.grad}
    extra = {"model.x": x3.detach().contiguous().numpy(), "model.g": x0.grad.contiguous().numpy(),
             "model.dlogits": logits.grad.contiguous().numpy()}
    return x3.detach().contiguous(), w, b, x0.grad.contiguous(), got, extra


def run_layer_case(inputs):
    x, w, b, g = inputs()
    c_in = x.shape[-1]
    layer = torch.nn.Sequential(torch.nn.Linear(c_in, 2 * c_in), torch.nn.ReLU(inplace=True)).train()
    with torch.no_grad():
        layer[0].weight.copy_(w)
        layer[0].bias.copy_(b)
    xx = x.clone().requires_grad_()
    y = layer(xx)
    y.backward(g)
    return x, w, b, g, {"y": y.detach(), "dw": layer[0].weight.grad, "db": layer[0].bias.grad, "dx": xx.grad}, {}


def main():
    fx = {"meta.names": np.asarray(Lc.FIXTURE_CASES)}
    d = {k: 0.0 for k in Lc.GATED}
    runs = (("model", run_model_case), ("edges", lambda: run_layer_case(Lc.edges_inputs)),
            ("c32", lambda: run_layer_case(lambda: Lc.width_inputs(32))), ("c64", lambda: run_layer_case(lambda: Lc.width_inputs(64))))
    for name, run in runs:
        x, w, b, g, got, extra = run()
        res = Lc.restate64(x, w, b, g)
        ag = Lc.autograd64(x, w, b, g)
        for k in Lc.GRADS:
            assert Lc.err(ag[k], res[k], res["S"][k]) <= 1e-12, (name, k)
        line = []
        for k in Lc.GATED:
            e = Lc.err(got[k], res[k], res["S"][k])
            assert np.isfinite(e), (name, k)
            d[k] = max(d[k], e)
            line.append(f"{k} {e:.2e}")
            fx[f"{name}.{k}"] = got[k].detach().numpy().astype(np.float32)
        kink = Lc.kink_distance(res)
        moved = float((got["y"].double().reshape(res["h"].shape) - res["h"].clamp(min=0)).abs().max())
        print(f"{name:6s} N {x.numel() // x.shape[-1]} " + " ".join(line) + f" kink {kink:.2e} float32 movement of y {moved:.2e}")
        assert kink > Lc.KINK_FACTOR * moved, (name, kink, moved)
        # the reference's float32 mask is the restatement's
        assert bool(((got["y"].reshape(res["h"].shape) > 0) == (res["h"] > 0)).all()), name
        fx[f"{name}.kink"], fx[f"{name}.moved"] = np.float64(kink), np.float64(moved)
        fx[f"{name}.inputs_sha256"] = np.asarray(Lc.regenerated_inputs_digest(name))
        fx.update(extra)
        if name == "edges":
            h = res["h"]
            assert bool((h[Lc.EDGES_ZERO_ROW, :8] == 0).all()) and bool((g[Lc.EDGES_ZERO_ROW, :8] != 0).all())
            assert bool((got["y"].reshape(h.shape)[Lc.EDGES_ZERO_ROW, :8] == 0).all())
            for c in (Lc.EDGES_DEAD, 200):
                assert bool((h[:, c] < 0).all()) and float(res["db"][c]) == 0.0 and bool((res["dw"][c] == 0).all())
                assert float(got["db"][c]) == 0.0 and bool((got["dw"][c] == 0).all())
            assert bool((h[:, 101] > 0).all()) and bool((h[:, 201] > 0).all())
    for k in Lc.GATED:
        fx[f"d_{k}"], fx[f"tol_{k}"] = np.float64(d[k]), np.float64(max(4 * d[k], Lc.TOL_FLOOR))
        print(f"d_{k} {d[k]:.3e} tol {max(4 * d[k], Lc.TOL_FLOOR):.3e}")
    np.savez_compressed(Lc.FIXTURE, **fx)
    print("wrote", Lc.FIXTURE, os.path.getsize(Lc.FIXTURE), "bytes")
    assert os.path.getsize(Lc.FIXTURE) < 1000000


if __name__ == "__main__":
    main()
