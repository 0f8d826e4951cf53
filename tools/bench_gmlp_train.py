#!/usr/bin/env python3
"""Stage 4's multi-axis gated-MLP layer in training mode (forward + backward) on the GPU against the torch-op composition:
python tools/bench_gmlp_train.py [--out FILE] [--reps N] [--hip-only] -> one JSON document (default profiles/gmlp_train_bench.json).

Shapes: 4 x 24 x 24 (the reference's training batch: four 192-pixel patches) and 16 x 64 x 80 (sixteen VGA images), as
(B, Hc, Wc) of the layer's input x0 [B,Hc,Wc,256].  Per shape, with the gradients of the parameters only and with dx0 as well:

* one step of the layer through the library -- `ops.gmlp_train_forward`, then `ops.gmlp_train_backward` (13 + 51 launches) -- and
  the same step by the float32 torch-op composition the tests state (tests/gmlp_train_common.py: _compose, the oracle's
  F.layer_norm, F.linear, F.gelu and the einsum over a 6-D view) under autograd, on leaves made once.  Both on the GPU, us per
  step between device events around `--reps` back-to-back steps after a warm-up, the two alternated three times, median and
  spread ((max - min) / median) of the three;
* the two library calls alone, timed the same way;
* the FLOPs of the matrix products (the channel products and the three token products per branch) and the achieved FLOP/s of the
  HIP step -- a whole-step rate that includes the launch gaps and the row kernels, not a kernel's share of peak;
* the 28 outputs of both paths against the float64 restatement of the tests, evaluated on the device, in the gates' measure, on
  the inputs of the tests' sweep: `against_float64`.  The suite gates the same at N = 65664 (1280-pixel slices,
  80-row column blocks, five groups per workgroup of the token-mix backward); the 16 x 64 x 80 run is the figure at the size timed.

`--hip-only`: the HIP steps alone, a few of them, for a kernel trace.  The exit status is 0 either way: DESIGN.md 7n records what
was found."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import ops                                                        # noqa: E402
from tests import gmlp_train_common as G                                        # noqa: E402

SHAPES = ((4, 24, 24), (16, 64, 80))
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gmlp_train_bench.json")


def gemm_flops(n, dx0):
    """Forward: dense1 (256 x 512), two branches of dense1 (256 x 512) + the token product (64 per element of [N,256]) + dense2
    (256 x 256), dense2 (512 x 256).  Backward: a weight gradient and an input gradient per product (the token product: dWt and
    dcn), with or without dx0: dn0 = dh0 W1 feeds the LayerNorm's gain and bias gradients either way."""
    fwd = 2 * n * (256 * 512 + 2 * (256 * 512 + 64 * 256 + 256 * 256) + 512 * 256)
    return 3 * fwd


def us_per_call(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def stats(v):
    med = float(np.median(v))
    return {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
            "spread": round((max(v) - min(v)) / med, 4)}


def accuracy(dev, shape):
    """The outputs of both paths against restate64 (evaluated on the device) in the gates' measure err(T) = max |T - T64| / S_T,
    on the inputs of the tests' shape sweep."""
    x0, p, g = G.sweep_case(shape, 900 + shape[0])
    x0, g, p = x0.to(dev), g.to(dev), {k: v.to(dev) for k, v in p.items()}
    res = G.restate64(x0, p, g)
    want = {k: res[k].cpu() for k in G.GATED}
    params = [p[k] for k in G.PARAMS]
    f = ops.gmlp_train_forward(x0, params)
    back = ops.gmlp_train_backward(g, x0, params, f.saved, want_dx0=True)
    got = dict({"d:" + k: t for k, t in zip(G.PARAMS, back.grads)}, y=f.y, dx0=back.dx0)
    y32, g32 = G.compose_f32(x0, p, g)
    got32 = dict(g32, y=y32)
    hip = {k: G.err(got[k], want[k], res["S"][k]) for k in G.GATED}
    comp = {k: G.err(got32[k], want[k], res["S"][k]) for k in G.GATED}
    worst = lambda d: max(d.items(), key=lambda kv: kv[1])      # noqa: E731
    return {"inputs": "tests/gmlp_train_common.py: sweep_case",
            "hip_err": {k: float("%.3g" % v) for k, v in hip.items()},
            "torch_composition_err": {k: float("%.3g" % v) for k, v in comp.items()},
            "hip_worst": [worst(hip)[0], float("%.3g" % worst(hip)[1])],
            "torch_composition_worst": [worst(comp)[0], float("%.3g" % worst(comp)[1])]}


def bench_shape(dev, b, hc, wc, reps, hip_only):
    n = b * hc * wc
    gen = torch.Generator(device=dev).manual_seed(n)
    x0 = (torch.randn((b, hc, wc, 256), device=dev, generator=gen) + 0.3).clamp(min=0)
    dy = torch.randn((b, hc, wc, 256), device=dev, generator=gen) / n
    p = {k: v.to(dev) for k, v in G.sweep_params(5)[0].items()}
    params = [p[k] for k in G.PARAMS]
    saved = torch.empty(ops.lib().balf_gmlp_train_saved_bytes(b, hc, wc), dtype=torch.uint8, device=dev)

    def fwd():
        return ops.gmlp_train_forward(x0, params, saved=saved)

    def bwd(dx0):
        return ops.gmlp_train_backward(dy, x0, params, saved, want_dx0=dx0)

    def hip(dx0):
        f = fwd()
        return f, bwd(dx0)

    out = {"shape": [b, hc, wc], "pixels": n, "repetitions": reps}
    if hip_only:
        for _ in range(reps):
            hip(True)
        torch.cuda.synchronize()
        return out
    for dx0 in (False, True):
        leaves = {k: p[k].clone().requires_grad_() for k in G.PARAMS}      # made once: a step pays for no copy
        xc = x0.clone().requires_grad_(dx0)

        def composed():
            for t in list(leaves.values()) + [xc]:
                t.grad = None
            y = G._compose(xc, leaves)
            y.backward(dy)
            return y.detach(), leaves["dense1.weight"].grad

        f, a = hip(dx0)
        y_c, dw1_c = composed()                                             # warm-up of both, and the check
        agree = {"y_max_abs_diff": float((f.y - y_c).abs().max()), "dW1_max_abs_diff": float((a.grads[2] - dw1_c).abs().max()),
                 "dW1_max_abs": float(dw1_c.abs().max())}
        del f, a, y_c, dw1_c
        times = {k: [] for k in ("hip", "torch_composition", "gmlp_forward", "gmlp_backward")}
        for _ in range(3):
            times["hip"].append(us_per_call(lambda: hip(dx0), reps))
            times["torch_composition"].append(us_per_call(composed, reps))
            times["gmlp_forward"].append(us_per_call(fwd, reps))
            times["gmlp_backward"].append(us_per_call(lambda: bwd(dx0), reps))
        st = {k: stats(v) for k, v in times.items()}
        sh, sc = st["hip"], st["torch_composition"]
        key = "with_dx0" if dx0 else "parameters_only"
        out[key] = {**st, "speedup": round(sc["median_us"] / sh["median_us"], 2),
                    "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]), "gemm_flops": gemm_flops(n, dx0),
                    "hip_achieved_TFLOP_per_s": round(gemm_flops(n, dx0) / (sh["median_us"] * 1e-6) / 1e12, 2),
                    "torch_achieved_TFLOP_per_s": round(gemm_flops(n, dx0) / (sc["median_us"] * 1e-6) / 1e12, 2), **agree}
        print(json.dumps({key: out[key], "shape": [b, hc, wc]}), flush=True)
    out["against_float64"] = accuracy(dev, (b, hc, wc))
    print(json.dumps({"against_float64": {k: out["against_float64"][k] for k in ("hip_worst", "torch_composition_worst")},
                      "shape": [b, hc, wc]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"metric": "stage 4's gMLP layer in training mode, forward + backward (balf_gmlp_train_*) vs the float32 torch-op "
                     "composition under autograd, device-event us per step",
           "device": torch.cuda.get_device_name(dev),
           "shapes": [bench_shape(dev, b, hc, wc, args.reps, args.hip_only) for b, hc, wc in SHAPES]}
    if args.out and not args.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
