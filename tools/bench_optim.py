#!/usr/bin/env python3
"""The optimiser step, A/B: balf_amd.optim.FusedAdam (one launch per group) against torch.optim.Adam(foreach=True)
and, where this torch build offers it, torch.optim.Adam(fused=True):  python tools/bench_optim.py [--out FILE] [--rounds N]
-> one JSON document (default profiles/optim_ab.json).

Per optimiser, in a process of its own, the processes alternating (`--rounds` rounds over all of them; median and spread
(max - min) / median of the rounds):

* `step()` alone, gradients in place, on the parameters of `TrainableHead` (6 tensors, 83 k elements) and of `TrainableStage4` (44
  tensors, 949 k): us per step between device events around `--reps` back-to-back steps -- the rate at which steps get through,
  whichever of host and device is slower -- and the host's own time for issuing them;
* the whole `utils.train_utils.train_head` step of `TrainableStage4` (two encodes of the frozen model, two heads forward, the
  loss, backward, `step()`, the read of the loss) at 4 x 24 x 24 and 16 x 64 x 80 feature pixels (4 x 3 x 192 x 192 and
  16 x 3 x 512 x 640 images: the shapes of tools/bench_stage4_train.py), wall us per call.

The comparison is between optimisers on the same tree.  `fused_not_slower` says per parameter set whether FusedAdam's median is at
most each of torch's: `utils.train_utils.build_optimizer` prefers the fused classes on that evidence.  The exit status is 0 either
way: DESIGN.md 7s records what was found."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "optim_ab.json")
VARIANTS = ("fused", "torch_foreach", "torch_fused")
TRAIN_SHAPES = ((4, 24, 24), (16, 64, 80))


def child(variant, reps, train_reps):
    import torch
    from balf_amd import arch
    from balf_amd.model import get_model
    from balf_amd.model.head_train import TrainableHead
    from balf_amd.model.stage4_train import TrainableStage4
    from balf_amd.optim import FusedAdam
    from balf_amd.utils import synth, train_utils

    dev = torch.device("cuda:0")

    def make(params):
        if variant == "fused":
            return FusedAdam(params, lr=1e-3)
        if variant == "torch_foreach":
            return torch.optim.Adam(params, lr=1e-3, foreach=True)
        return torch.optim.Adam(params, lr=1e-3, fused=True)

    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(2))
    model = model.eval().to(dev)
    out = {"variant": variant, "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "step_only": {}, "train_head": {}}

    for name, cls in (("head", TrainableHead), ("stage4", TrainableStage4)):
        params = list(cls.from_model(model).parameters())
        try:
            opt = make(params)
        except (RuntimeError, ValueError) as e:                      # fused=True not offered by this build
            out["unavailable"] = str(e)
            print(json.dumps(out), flush=True)
            return
        gen = torch.Generator(device=dev).manual_seed(len(params))
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
        for _ in range(20):                                          # state, caches, the allocator: untimed
            opt.step()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            opt.step()
        host = time.perf_counter() - t0
        stop.record()
        torch.cuda.synchronize()
        out["step_only"][name] = {"tensors": len(params), "elements": sum(p.numel() for p in params),
                                  "us_per_step": start.elapsed_time(stop) * 1e3 / reps, "host_us_per_step": host * 1e6 / reps}

    for b, hc, wc in TRAIN_SHAPES:
        stage = TrainableStage4.from_model(model)
        opt = make(list(stage.parameters()))
        gen = torch.Generator(device=dev).manual_seed(b * hc * wc)
        images = [torch.rand((b, 3, 8 * hc, 8 * wc), device=dev, generator=gen) for _ in range(2)]
        heat = [(torch.rand((b, 1, 8 * hc, 8 * wc), device=dev, generator=gen) < 0.01).float() for _ in range(2)]
        loader = [(images[0], images[1], heat[0], heat[1], None, None)]
        n = max(3, train_reps // (4 if b * hc * wc > 10000 else 1))
        for _ in range(3):
            train_utils.train_head(loader, model, stage, opt, dev, noise=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            train_utils.train_head(loader, model, stage, opt, dev, noise=False)     # (ends with the read of the loss)
        out["train_head"][f"{b}x{hc}x{wc}"] = {"calls": n, "us_per_step": (time.perf_counter() - t0) * 1e6 / n}
    print(json.dumps(out), flush=True)


def stats(v):
    med = float(np.median(v))
    return {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
            "spread": round((max(v) - min(v)) / med, 4), "rounds": [round(x, 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--train-reps", type=int, default=40)
    ap.add_argument("--child", choices=VARIANTS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.train_reps)
        return
    runs = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for v in VARIANTS:
            if runs[v] and "unavailable" in runs[v][0]:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, "--reps", str(args.reps), "--train-reps",
                                str(args.train_reps)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"bench_optim: the {v} process ended with status {r.returncode}")
            runs[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"metric": "optimizer.step() of Adam over the trainable parameters (device-event us per step, back-to-back steps, and the "
                     "host's us for issuing one) and the whole train_head step of TrainableStage4 (wall us per call); one process "
                     "per optimiser and round, alternating; median over the rounds",
           "device": runs["fused"][0]["device"], "torch": runs["fused"][0]["torch"], "rounds": args.rounds, "variants": {}}
    for v in VARIANTS:
        if "unavailable" in runs[v][0]:
            doc["variants"][v] = {"unavailable": runs[v][0]["unavailable"]}
            continue
        first = runs[v][0]
        doc["variants"][v] = {
            "step_only": {k: {"tensors": first["step_only"][k]["tensors"], "elements": first["step_only"][k]["elements"],
                              "step": stats([r["step_only"][k]["us_per_step"] for r in runs[v]]),
                              "host": stats([r["step_only"][k]["host_us_per_step"] for r in runs[v]])} for k in first["step_only"]},
            "train_head": {k: stats([r["train_head"][k]["us_per_step"] for r in runs[v]]) for k in first["train_head"]}}
    have = [v for v in VARIANTS[1:] if "step_only" in doc["variants"][v]]
    fused = doc["variants"]["fused"]
    doc["fused_not_slower"] = {k: all(fused["step_only"][k]["step"]["median_us"] <= doc["variants"][v]["step_only"][k]["step"]["median_us"]
                                      for v in have) for k in fused["step_only"]}
    doc["speedup_over"] = {v: {k: round(doc["variants"][v]["step_only"][k]["step"]["median_us"] / fused["step_only"][k]["step"]["median_us"], 2)
                               for k in fused["step_only"]} for v in have}
    doc["fused_step_share_of_stage4_train_head_step"] = {
        k: round(fused["step_only"]["stage4"]["step"]["median_us"] / fused["train_head"][k]["median_us"], 4) for k in fused["train_head"]}
    print(json.dumps(doc, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
