#!/usr/bin/env python3
"""Record tests/golden/gmlp_train.npz from the REFERENCE's own modules and PyTorch's autograd on the CPU.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    python tests/golden/make_gmlp_train_golden.py

Case ``model``: the reference's MLP_MA_DECODER with synth.synthetic_state_dict(0) in .train() on the seeded 2 x 3 x 64 x 64 image
of tests/head_train_common.py: model_inputs.  Forward-pre-hooks capture x0 at down4.residual_split_head_multi_axis_gmlp_layer, y at
down4.residual_channel_attention_block and x2 at down4.conv2 (retain_grad all three), and the seeded dlogits goes back with
(logits * g).sum().backward().  Stored: x0 and dy = y.grad (the inputs), the reference's float32 y and 26 parameter gradients,
and ``dx0_full`` = x0.grad, which holds all three paths into x0 (the layer, its shortcut and the long shortcut); dx0 of the layer
alone, x0.grad - x2.grad, enters d_T only.  Hc = Wc = 8 there: the grid and the block map coincide, so
this case pins the real weight distribution only.  Cases ``layout`` and ``edges``: gmlp_train_common.layout_inputs / edges_inputs
through the reference's ResidualSplitHeadMultiAxisGmlpLayer(256, (8, 8), (8, 8)), constructed on its own.  Also stored: a SHA-256
of the inputs that are regenerated instead of stored, and the gates: d_T = the largest err (gmlp_train_common.err, against the
float64 restatement) of the reference's own float32 result over the cases, tol_T = max(4 * d_T, 1.1e-6).  Large results are
recorded on some rows only (gmlp_train_common.recorded_part).  Nothing of the reference is committed: the fixture holds numbers
only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_model                                      # noqa: E402  (puts the reference on the path)
from balf.model.mlp_ma_decoder import ResidualSplitHeadMultiAxisGmlpLayer           # noqa: E402  (reference)
from tests import gmlp_train_common as Gc                                           # noqa: E402


def layer_grads(layer):
    own = dict(layer.named_parameters())
    return {"d:" + k: own[k].grad for k in Gc.PARAMS}


def run_model_case():
    image, p, dlogits, _ = Gc.model_inputs()
    m, _ = ref_model(0)
    m.train()
    seen = {}

    def keep(name):
        def hook(_module, args):
            args[0].retain_grad()
            seen[name] = args[0]
        return hook

    handles = [m.down4.residual_split_head_multi_axis_gmlp_layer.register_forward_pre_hook(keep("x0")),
               m.down4.residual_channel_attention_block.register_forward_pre_hook(keep("y")),
               m.down4.conv2.register_forward_pre_hook(keep("x2"))]
    out = m(image)
    for h in handles:
        h.remove()
    (out["logits"] * dlogits).sum().backward()
    x0, y, x2 = seen["x0"], seen["y"], seen["x2"]
    got = dict(layer_grads(m.down4.residual_split_head_multi_axis_gmlp_layer), y=y.detach())
    got["dx0"] = (x0.grad.double() - x2.grad.double())          # the layer's own share, exact to float64
    extra = {"model.dx0_full": Gc.recorded_part(x0.grad).contiguous().numpy()}
    return x0.detach().contiguous(), p, y.grad.contiguous(), got, extra


def run_layer_case(inputs):
    x0, p, g = inputs()
    layer = ResidualSplitHeadMultiAxisGmlpLayer(256, (8, 8), (8, 8)).train()
    own = dict(layer.named_parameters())
    with torch.no_grad():
        for k in Gc.PARAMS:
            own[k].copy_(p[k])
    xx = x0.clone().requires_grad_()
    y = layer(xx)
    y.backward(g)
    return x0, p, g, dict(layer_grads(layer), y=y.detach(), dx0=xx.grad), {}


def main():
    torch.manual_seed(0)
    fx = {"meta.names": np.asarray(Gc.FIXTURE_CASES)}
    d = {k: 0.0 for k in Gc.GATED}
    runs = (("model", run_model_case), ("layout", lambda: run_layer_case(Gc.layout_inputs)),
            ("edges", lambda: run_layer_case(Gc.edges_inputs)))
    for name, run in runs:
        x0, p, g, got, extra = run()
        res = Gc.restate64(x0, p, g)
        ag = Gc.autograd64(x0, p, g)
        for k in Gc.GRADS:
            assert Gc.err(ag[k], res[k], res["S"][k]) <= 1e-12, (name, k)
        line = []
        for k in Gc.GATED:
            e = Gc.err(got[k], res[k], res["S"][k])
            assert np.isfinite(e), (name, k)
            d[k] = max(d[k], e)
            line.append(f"{k} {e:.2e}")
            if not (name == "model" and k == "dx0"):            # stored as dx0_full
                fx[f"{name}.{k}"] = Gc.recorded_part(got[k].detach()).numpy().astype(np.float32)
        print(f"{name:6s} N {x0.numel() // 256} " + " ".join(line))
        fx[f"{name}.inputs_sha256"] = np.asarray(Gc.regenerated_inputs_digest(name))
        fx.update(extra)
        if name == "model":
            fx["model.x0"], fx["model.dy"] = x0.numpy(), g.numpy()
        if name == "edges":
            b, hc, wc = Gc.EDGES_SHAPE
            xh = (x0[Gc.EDGES_CONST_ROW].double() - x0[Gc.EDGES_CONST_ROW].double().mean())
            assert bool((xh == 0).all())
            assert res["S"]["d:grid_gmlp_layer.grid_gating_unit.norm.weight"] == 0.0     # var = 0 on every pixel of the gating norm
            h0, hb = res["h0"], res["hb"][1]
            assert float(h0.max()) > 8 and float(h0.min()) < -8 and float(hb.max()) > 8 and float(hb.min()) < -8
    for k in Gc.GATED:
        fx[f"d_{k}"], fx[f"tol_{k}"] = np.float64(d[k]), np.float64(max(4 * d[k], Gc.TOL_FLOOR))
        print(f"d_{k} {d[k]:.3e} tol {max(4 * d[k], Gc.TOL_FLOOR):.3e}")
    np.savez_compressed(Gc.FIXTURE, **fx)
    print("wrote", Gc.FIXTURE, os.path.getsize(Gc.FIXTURE), "bytes")
    assert os.path.getsize(Gc.FIXTURE) < 1000000


if __name__ == "__main__":
    main()
