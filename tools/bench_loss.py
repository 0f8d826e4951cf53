#!/usr/bin/env python3
"""detector_loss on the GPU against the torch-op composition: python tools/bench_loss.py [--out FILE] [--reps N] [--dry]
-> one JSON document.

Shapes: 64 x 256 x 256 (the loader's batch: logits [64,65,32,32]) and 32 x 1088 x 1920 (logits [32,65,136,240]); a valid
mask and a noise tensor are handed in (the whole contract).  Per shape, with and without the gradient:

* `ops.detector_loss` (balf_detector_loss, four launches) and the same quantity by the float32 torch-op composition of the
  tests (tests/detector_loss_common.py: compose_f32, the reference's statements with the noise handed in; its gradient through
  autograd), both on the GPU, µs per call between device events around `--reps` back-to-back calls after a warm-up, the two
  alternated three times, median and spread ((max - min) / median) of the three;
* the bytes the call must move (the byte budget of DESIGN §7k: logits, key-point map, mask and noise read once, the cell
  masks written and read once, the gradient written once) and the achieved bytes/s = those bytes over the call's time -- a
  whole-call rate (it includes the launch gaps of the four kernels), not a kernel's share of peak;
* both losses checked against each other.

`--dry`: the byte counts only, no GPU.  Exit status 1 if the HIP call is slower than the composition anywhere."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import ops                                                        # noqa: E402
from tests import detector_loss_common as D                                     # noqa: E402

SHAPES = ((64, 256, 256), (32, 1088, 1920))


def budget_bytes(b, h, w, grad):
    cells = b * (h // 8) * (w // 8)
    parts = {"logits": 65 * 4 * cells, "keypoint_map": 64 * 4 * cells, "valid_mask": 64 * 4 * cells, "noise": 65 * 4 * cells,
             "cell_masks_write_read": 8 * cells, "dlogits": 65 * 4 * cells if grad else 0}
    return parts, sum(parts.values())


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


def bench_shape(dev, b, h, w, reps):
    hc, wc = h // 8, w // 8
    g = torch.Generator(device=dev).manual_seed(b + h)
    logits = torch.randn((b, 65, hc, wc), device=dev, generator=g) * 4
    kp = (torch.rand((b, 1, h, w), device=dev, generator=g) < 0.002).float()
    vm = (torch.rand((b, 1, h, w), device=dev, generator=g) >= 0.0005).float()
    noise = torch.rand((b, 65, hc, wc), device=dev, generator=g) * 0.1
    out = {"shape": [b, h, w], "logits": [b, 65, hc, wc], "repetitions": reps}
    for grad in (False, True):
        def hip():
            return ops.detector_loss(logits, kp, vm, noise, want_grad=grad)

        def composed():
            return D.compose_f32(logits, kp, vm, noise, want_grad=grad)

        a, c = hip(), composed()                                          # warm-up of both, and the check
        c_loss, c_grad = (c if grad else (c, None))
        agree = {"loss_hip": float(a.loss), "loss_composition": float(c_loss),
                 "loss_rel_diff": abs(float(a.loss) - float(c_loss)) / max(abs(float(c_loss)), 1.0)}
        if grad:
            agree["grad_max_abs_diff"] = float((a.dlogits - c_grad).abs().max())
        del a, c, c_grad
        t_hip, t_comp = [], []
        for _ in range(3):
            t_hip.append(us_per_call(hip, reps))
            t_comp.append(us_per_call(composed, max(1, reps // 4)))
        parts, total = budget_bytes(b, h, w, grad)
        sh, sc = stats(t_hip), stats(t_comp)
        key = "with_dlogits" if grad else "loss_only"
        out[key] = {"hip": sh, "torch_composition": sc, "speedup": round(sc["median_us"] / sh["median_us"], 2),
                    "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]), "budget_bytes": total, "budget_parts": parts,
                    "hip_achieved_TB_per_s": round(total / (sh["median_us"] * 1e-6) / 1e12, 3), **agree}
        print(json.dumps({key: out[key], "shape": [b, h, w]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    if args.dry:
        for b, h, w in SHAPES:
            print(json.dumps({"shape": [b, h, w], "loss_only": budget_bytes(b, h, w, False)[1],
                              "with_dlogits": budget_bytes(b, h, w, True)[1]}))
        return
    dev = torch.device("cuda:0")
    doc = {"metric": "detector_loss (balf_detector_loss) vs the float32 torch-op composition, device-event us per call",
           "device": torch.cuda.get_device_name(dev), "shapes": [bench_shape(dev, b, h, w, args.reps) for b, h, w in SHAPES]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ok = all(s[k]["hip_not_slower"] for s in doc["shapes"] for k in ("loss_only", "with_dlogits"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
