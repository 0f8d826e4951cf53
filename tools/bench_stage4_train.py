#!/usr/bin/env python3
"""All of stage 4 and the head in training mode (forward + backward of model.stage4_train.TrainableStage4) on the GPU against the
torch-op composition: python tools/bench_stage4_train.py [--out FILE] [--reps N] [--hip-only] -> one JSON document (default
profiles/stage4_train_bench.json).

Shapes: 4 x 24 x 24 (the reference's training batch: four 192-pixel patches) and 16 x 64 x 80 (sixteen VGA images), as
(B, Hc, Wc) of the stage's input x3 [B,Hc,Wc,128].  Per shape, with the gradients of the 44 parameter tensors only and with
x3.grad as well:

* one step of `TrainableStage4` -- `stage(x3)["logits"].backward(dlogits)`: down4.conv.0 + ReLU, the gated-MLP layer, the
  channel-attention block and the head on the library, their `autograd.Function`s chained by torch -- and the same step by the
  float32 torch-op composition the tests state (tests/linrelu_train_common.py: stage4_compose, then the head's F.linear, F.relu,
  F.linear, F.batch_norm) under autograd, on leaves made once.  Both on the GPU, us per step between device events around
  `--reps` back-to-back steps; every path of both configurations runs an untimed window first, then three rounds alternate all of
  them; median and spread ((max - min) / median) of the three;
* the new layer alone (`ops.linrelu_train_forward` + `ops.linrelu_train_backward`), timed the same way;
* the four outputs of the new layer on both paths against the float64 restatement of the tests, evaluated on the device, in the
  gates' measure, on the inputs of the tests' sweep: `against_float64`.  The suite gates the same at N = 65537 (1280-pixel
  slices, 80-row blocks); the 16 x 64 x 80 run (N = 81920) is the figure at the size that is timed.

`--hip-only`: the HIP steps alone, a few of them, for a kernel trace.  The exit status is 0 either way: DESIGN.md 7o records what
was found."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch, ops                                                  # noqa: E402
from balf_amd.model import get_model                                            # noqa: E402
from balf_amd.model.stage4_train import TrainableStage4                         # noqa: E402
from balf_amd.utils import synth                                                # noqa: E402
from tests import gmlp_train_common as G                                        # noqa: E402
from tests import head_train_common as H                                        # noqa: E402
from tests import linrelu_train_common as L                                     # noqa: E402
from tests import rcab_train_common as R                                        # noqa: E402

SHAPES = ((4, 24, 24), (16, 64, 80))
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage4_train_bench.json")


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


def accuracy(dev, n):
    """The new layer's outputs on both paths against restate64 (evaluated on the device) in the gates' measure, c_in = 128."""
    x, w, b, g = (t.to(dev) for t in L.sweep_case(n, 128, 900))
    res = L.restate64(x, w, b, g)
    y = ops.linrelu_train_forward(x, w, b).y
    back = ops.linrelu_train_backward(g, y, x, w, want_dx=True)
    got = {"y": y, "dw": back.dweight, "db": back.dbias, "dx": back.dx}
    y32, g32 = L.compose_f32(x, w, b, g)
    got32 = dict(g32, y=y32)
    want = {k: res[k].cpu() for k in L.GATED}
    return {"inputs": "tests/linrelu_train_common.py: sweep_case",
            "hip_err": {k: float("%.3g" % L.err(got[k], want[k], res["S"][k])) for k in L.GATED},
            "torch_composition_err": {k: float("%.3g" % L.err(got32[k], want[k], res["S"][k])) for k in L.GATED}}


def bench_shape(dev, model, sd, b, hc, wc, reps, hip_only):
    n = b * hc * wc
    gen = torch.Generator(device=dev).manual_seed(n)
    x3 = torch.randn((b, hc, wc, 128), device=dev, generator=gen)
    dlogits = torch.randn((b, 65, hc, wc), device=dev, generator=gen) / n
    stage = TrainableStage4.from_model(model)
    w0, b0 = (t.detach() for t in stage.conv0_parameters())
    g0 = torch.randn((b, hc, wc, 256), device=dev, generator=gen) / n

    def hip(dx):
        xs = x3.requires_grad_(dx)
        for p in stage.parameters():
            p.grad = None
        xs.grad = None
        logits = stage(xs, want_prob=False)["logits"]
        logits.backward(dlogits)
        return logits.detach()

    def layer(dx):
        y = ops.linrelu_train_forward(x3.detach(), w0, b0).y
        return ops.linrelu_train_backward(g0, y, x3.detach(), w0, want_dx=dx)

    out = {"shape": [b, hc, wc], "pixels": n, "repetitions": reps}
    if hip_only:
        for _ in range(reps):
            hip(True)
        torch.cuda.synchronize()
        return out
    hp, running = H.params_of(sd)

    def composition(dx):
        c0 = [t.to(dev).clone().requires_grad_() for t in L.params_of(sd)]           # made once: a step pays for no copy
        gl = {k: v.to(dev).requires_grad_() for k, v in G.params_of(sd).items()}
        rl = {k: v.to(dev).requires_grad_() for k, v in R.params_of(sd).items()}
        hl = {k: v.to(dev).requires_grad_() for k, v in hp.items()}
        rm, rv = running[0].to(dev).clone(), running[1].to(dev).clone()
        leaves = c0 + list(gl.values()) + list(rl.values()) + list(hl.values())
        xc = x3.detach().clone().requires_grad_(dx)

        def composed():
            for t in leaves + [xc]:
                t.grad = None
            x2 = L.stage4_compose(xc, c0[0], c0[1], gl, rl)
            z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
            logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
            logits.backward(dlogits)
            return logits.detach(), c0[0].grad

        return composed

    # both configurations are set up, checked and run for an untimed window before any of them is timed, and the three rounds walk
    # through all of them: at 4 x 24 x 24 a step is 115 launches in ~1.2 ms, and what the host did just before shows in it
    configs = {False: composition(False), True: composition(True)}
    agree, times = {}, {}
    for dx, composed in configs.items():
        a, (c, dw_c) = hip(dx), composed()
        agree[dx] = {"logits_max_abs_diff": float((a - c).abs().max()),
                     "dconv0_weight_max_abs_diff": float((stage.conv0.weight.grad - dw_c).abs().max()),
                     "dconv0_weight_max_abs": float(dw_c.abs().max())}
        del a, c, dw_c
        for fn in (lambda: hip(dx), composed, lambda: layer(dx)):
            us_per_call(fn, reps)
        times[dx] = {k: [] for k in ("hip", "torch_composition", "linrelu_layer")}
    for _ in range(3):
        for dx, composed in configs.items():
            times[dx]["hip"].append(us_per_call(lambda: hip(dx), reps))
            times[dx]["torch_composition"].append(us_per_call(composed, reps))
            times[dx]["linrelu_layer"].append(us_per_call(lambda: layer(dx), reps))
    for dx in configs:
        st = {k: stats(v) for k, v in times[dx].items()}
        sh, sc = st["hip"], st["torch_composition"]
        key = "with_dx" if dx else "parameters_only"
        out[key] = {**st, "speedup": round(sc["median_us"] / sh["median_us"], 2),
                    "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]),
                    "linrelu_share_of_hip_step": round(st["linrelu_layer"]["median_us"] / sh["median_us"], 4), **agree[dx]}
        print(json.dumps({key: out[key], "shape": [b, hc, wc]}), flush=True)
    x3.requires_grad_(False)
    out["against_float64"] = accuracy(dev, n)
    print(json.dumps({"against_float64": out["against_float64"], "shape": [b, hc, wc]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth.synthetic_state_dict(2)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    doc = {"metric": "all of stage 4 and the head in training mode, forward + backward (TrainableStage4) vs the float32 torch-op "
                     "composition under autograd, device-event us per step",
           "device": torch.cuda.get_device_name(dev),
           "shapes": [bench_shape(dev, model, sd, b, hc, wc, args.reps, args.hip_only) for b, hc, wc in SHAPES]}
    if args.out and not args.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
