#!/usr/bin/env python3
"""Stages 3-4 and the head in training mode (forward + backward of model.stage3_train.TrainableStage3) on the GPU against the
torch-op composition: python tools/bench_stage3_train.py [--out FILE] [--reps N] [--hip-only] -> one JSON document (default
profiles/stage3_train_bench.json).

Shapes: the batches of tools/bench_stage4_train.py, 4 x 24 x 24 (the reference's training batch: four 192-pixel patches) and
16 x 64 x 80 (sixteen VGA images) as (B, Hc, Wc) of stage 4; the stage's input x2s is [B,2Hc,2Wc,64].  Per shape, with the
gradients of the 82 parameter tensors only and with x2s.grad as well:

* one step of `TrainableStage3` -- `stage(x2s)["logits"].backward(dlogits)`: down3.conv.0 + ReLU, the gated-MLP layer and the
  channel-attention block at C = 128, the 2 x 2 max-pool, then all of stage 4 and the head, on the library, their
  `autograd.Function`s chained by torch -- and the same step by the float32 torch-op composition the tests state
  (tests/stage3_train_common.py: stage_compose, then the head's F.linear, F.relu, F.linear, F.batch_norm) under autograd, on
  leaves made once.  Both on the GPU, us per step between device events around `--reps` back-to-back steps; every path of both
  configurations runs an untimed window first, then three rounds alternate all of them; median and spread ((max - min) / median)
  of the three;
* stage 3 alone on the library (the five units from x2s to x3 and back, the gradient at x3 given), timed the same way, and its
  share of the step.

`--hip-only`: the HIP steps alone, a few of them, for a kernel trace.  The exit status is 0 either way: DESIGN.md 7x records what
was found."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch                                                       # noqa: E402
from balf_amd.model import get_model                                            # noqa: E402
from balf_amd.model.stage3_train import TrainableStage3                         # noqa: E402
from balf_amd.utils import synth                                                # noqa: E402
from tests import head_train_common as H                                        # noqa: E402
from tests import stage3_train_common as Sc                                     # noqa: E402

SHAPES = ((4, 24, 24), (16, 64, 80))
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage3_train_bench.json")


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


class _Stage3Only(torch.nn.Module):
    """TrainableStage3 with the identity in place of stage 4 and the head: what its forward hands to ``stage4`` comes back."""

    def forward(self, x3, want_prob=True):
        return {"logits": x3}


def bench_shape(dev, model, sd, b, hc, wc, reps, hip_only):
    n = b * hc * wc
    gen = torch.Generator(device=dev).manual_seed(n)
    x2s = torch.randn((b, 2 * hc, 2 * wc, 64), device=dev, generator=gen)
    dlogits = torch.randn((b, 65, hc, wc), device=dev, generator=gen) / n
    dx3 = torch.randn((b, hc, wc, 128), device=dev, generator=gen) / n
    stage = TrainableStage3.from_model(model)
    alone = TrainableStage3.from_model(model)
    alone.stage4 = _Stage3Only()

    def step(module, g, dx):
        xs = x2s.requires_grad_(dx)
        for p in module.parameters():
            p.grad = None
        xs.grad = None
        logits = module(xs, want_prob=False)["logits"]
        logits.backward(g)
        return logits.detach()

    out = {"shape": [b, hc, wc], "stage3_pixels": 4 * n, "repetitions": reps}
    if hip_only:
        for _ in range(reps):
            step(stage, dlogits, True)
        torch.cuda.synchronize()
        return out
    sp = Sc.stage_params(sd)

    def composition(dx):
        def leaf(t):
            return t.to(dev).clone().requires_grad_()                               # made once: a step pays for no copy
        leaves = {s: (tuple(leaf(t) for t in sp[s][0]), {k: leaf(v) for k, v in sp[s][1].items()},
                      {k: leaf(v) for k, v in sp[s][2].items()}) for s in (3, 4)}
        hl = {k: leaf(v) for k, v in sp["head"].items()}
        rm, rv = sp["running"][0].to(dev).clone(), sp["running"][1].to(dev).clone()
        flat = Sc._leaf_list(leaves, hl)
        xc = x2s.detach().clone().requires_grad_(dx)

        def composed():
            for t in flat + [xc]:
                t.grad = None
            x2 = Sc.stage_compose(xc, leaves)
            z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
            logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
            logits.backward(dlogits)
            return logits.detach(), leaves[3][0][0].grad

        return composed

    configs = {False: composition(False), True: composition(True)}
    agree, times = {}, {}
    w3 = dict(stage.down3.named_parameters())["conv.0.weight"]
    for dx, composed in configs.items():
        a, (c, dw_c) = step(stage, dlogits, dx), composed()
        agree[dx] = {"logits_max_abs_diff": float((a - c).abs().max()),
                     "dconv0_weight_max_abs_diff": float((w3.grad - dw_c).abs().max()),
                     "dconv0_weight_max_abs": float(dw_c.abs().max())}
        del a, c, dw_c
        for fn in (lambda: step(stage, dlogits, dx), composed, lambda: step(alone, dx3, dx)):
            us_per_call(fn, reps)
        times[dx] = {k: [] for k in ("hip", "torch_composition", "stage3_alone")}
    for _ in range(3):
        for dx, composed in configs.items():
            times[dx]["hip"].append(us_per_call(lambda: step(stage, dlogits, dx), reps))
            times[dx]["torch_composition"].append(us_per_call(composed, reps))
            times[dx]["stage3_alone"].append(us_per_call(lambda: step(alone, dx3, dx), reps))
    for dx in configs:
        st = {k: stats(v) for k, v in times[dx].items()}
        sh, sc = st["hip"], st["torch_composition"]
        key = "with_dx" if dx else "parameters_only"
        out[key] = {**st, "speedup": round(sc["median_us"] / sh["median_us"], 2),
                    "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]),
                    "stage3_share_of_hip_step": round(st["stage3_alone"]["median_us"] / sh["median_us"], 4), **agree[dx]}
        print(json.dumps({key: out[key], "shape": [b, hc, wc]}), flush=True)
    x2s.requires_grad_(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth.synthetic_state_dict(2)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    doc = {"metric": "stages 3-4 and the head in training mode, forward + backward (TrainableStage3) vs the float32 torch-op "
                     "composition under autograd, device-event us per step",
           "device": torch.cuda.get_device_name(dev),
           "shapes": [bench_shape(dev, model, sd, b, hc, wc, args.reps, args.hip_only) for b, hc, wc in SHAPES]}
    if args.out and not args.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
