#!/usr/bin/env python3
"""Record tests/golden/head_train.npz from the REFERENCE's own modules and PyTorch's autograd on the CPU.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_head_train_golden.py

Case ``model``: the reference's MLP_MA_DECODER with synth.synthetic_state_dict(0) in .train() on the seeded 2 x 3 x 64 x 64 image
of tests/head_train_common.py: model_inputs; a forward-pre-hook on down4.conv2 captures x2 (retain_grad), the seeded dlogits g
goes back with (logits * g).sum().backward().  Case ``edges``: head_train_common.edges_inputs through an nn.Linear and the
reference's DetectorHead class in .train().  Stored: x2 of case ``model`` (the other inputs are seeded or the checkpoint's, see
head_train_common), the reference's float32 logits, six parameter gradients, dx2 and updated running statistics, the distance of
the pre-activations from the ReLU kink, a SHA-256 of the inputs that are regenerated instead of stored (a drift of the seeded
generators or of synth.synthetic_state_dict must fail the host test, not silently pair new inputs with old results), and the gates: d_T = the largest err (head_train_common.err, against the float64
restatement) of the reference's own float32 result over the cases, tol_T = max(4 * d_T, 1.1e-6).  Nothing of the reference is
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
from balf.model.decoder import DetectorHead                                         # noqa: E402  (reference)
from tests import head_train_common as H                                            # noqa: E402

_REF_NAMES = {"dw2": "conv2.weight", "db2": "conv2.bias", "dwd": "dense.weight", "dbd": "dense.bias", "dgamma": "norm.weight",
              "dbeta": "norm.bias"}


def run_model_case():
    image, p, dlogits, running = H.model_inputs()
    m, _ = ref_model(0)
    m.train()
    seen = {}

    def hook(_module, args):
        args[0].retain_grad()
        seen["x2"] = args[0]

    handle = m.down4.conv2.register_forward_pre_hook(hook)
    out = m(image)
    handle.remove()
    (out["logits"] * dlogits).sum().backward()
    grads = {"dw2": m.down4.conv2.weight.grad, "db2": m.down4.conv2.bias.grad, "dwd": m.detector_head.dense.weight.grad,
             "dbd": m.detector_head.dense.bias.grad, "dgamma": m.detector_head.norm.weight.grad,
             "dbeta": m.detector_head.norm.bias.grad, "dx2": seen["x2"].grad}
    bn = m.detector_head.norm
    assert int(bn.num_batches_tracked) == 1
    return (seen["x2"].detach().contiguous(), p, dlogits, running, out["logits"].detach(), out["prob"].detach(), grads,
            (bn.running_mean.detach().clone(), bn.running_var.detach().clone()))


def run_edges_case():
    x2, p, dlogits, running = H.edges_inputs()
    conv2 = torch.nn.Linear(256, 256)
    head = DetectorHead(256, 8).train()
    with torch.no_grad():
        conv2.weight.copy_(p["w2"]); conv2.bias.copy_(p["b2"])
        head.dense.weight.copy_(p["wd"]); head.dense.bias.copy_(p["bd"])
        head.norm.weight.copy_(p["gamma"]); head.norm.bias.copy_(p["beta"])
        head.norm.running_mean.copy_(running[0]); head.norm.running_var.copy_(running[1])
    x = x2.clone().requires_grad_()
    out = head(conv2(x).permute(0, 3, 1, 2))
    (out["logits"] * dlogits).sum().backward()
    grads = {"dw2": conv2.weight.grad, "db2": conv2.bias.grad, "dwd": head.dense.weight.grad, "dbd": head.dense.bias.grad,
             "dgamma": head.norm.weight.grad, "dbeta": head.norm.bias.grad, "dx2": x.grad}
    return (x2, p, dlogits, running, out["logits"].detach(), out["prob"].detach(), grads,
            (head.norm.running_mean.detach().clone(), head.norm.running_var.detach().clone()))


def main():
    torch.manual_seed(0)
    fx = {"meta.names": np.asarray(H.FIXTURE_CASES)}
    d = {k: 0.0 for k in H.GATED}
    for name, run in (("model", run_model_case), ("edges", run_edges_case)):
        x2, p, dlogits, running, logits, prob, grads, running_new = run()
        r = H.restate64(x2, p, dlogits, running=running)
        ag = H.autograd64(x2, p, dlogits)
        for k in H.GRADS:
            assert H.err(ag[k], r[k], r["S"][k]) <= 1e-12, (name, k)
        kink = H.kink_distance(r["h"])
        assert kink >= H.KINK_MARGIN, (name, kink)
        got = dict(grads, logits=logits, running_mean=running_new[0], running_var=running_new[1])
        line = []
        for k in H.GATED:
            e = H.err(got[k], r[k], r["S"][k])
            d[k] = max(d[k], e)
            line.append(f"{k} {e:.2e}")
            fx[f"{name}.{k}"] = got[k].numpy().astype(np.float32)
        prob_err = float((prob.double() - r["prob"]).abs().max())
        print(f"{name:6s} N {x2.numel() // 256} kink {kink:.2e} prob {prob_err:.2e} " + " ".join(line))
        fx[f"{name}.kink"] = np.float64(kink)
        fx[f"{name}.inputs_sha256"] = np.asarray(H.regenerated_inputs_digest(name))
        if name == "model":
            fx["model.x2"] = x2.numpy()
        else:
            zero = r["h"].reshape(*H.EDGES_SHAPE, 256)
            assert all(bool((zero[at][:8] == 0).all()) for at in H.EDGES_ZERO_ROWS)
            mean, var = r["mean"][H.EDGES_SHIFTED], r["var"][H.EDGES_SHIFTED]
            assert float(mean * mean / var) > 1e3, float(mean * mean / var)
    for k in H.GATED:
        fx[f"d_{k}"], fx[f"tol_{k}"] = np.float64(d[k]), np.float64(max(4 * d[k], H.TOL_FLOOR))
        print(f"d_{k} {d[k]:.3e} tol {max(4 * d[k], H.TOL_FLOOR):.3e}")
    np.savez_compressed(H.FIXTURE, **fx)
    print("wrote", H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes")
    assert os.path.getsize(H.FIXTURE) < 1 << 20


if __name__ == "__main__":
    main()
