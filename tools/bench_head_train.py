#!/usr/bin/env python3
"""The training-mode head (forward + backward) on the GPU against the torch-op composition:
python tools/bench_head_train.py [--out FILE] [--reps N] [--hip-only] -> one JSON document.

Shapes: 4 x 24 x 24 (the reference's training batch: four 192-pixel patches) and 16 x 64 x 80 (sixteen VGA images), as
(B, Hc, Wc) of the stage-4 features [B,Hc,Wc,256].  Per shape:

* `ops.head_train_forward` + `ops.head_train_backward` (balf_head_train_forward / balf_head_train_backward: 5 + 12 launches, 13 with dx2,
  prob not requested, running statistics updated, dx2 requested or not) and the same step by the float32 torch-op composition
  the tests state (tests/head_train_common.py: compose_f32 -- F.linear, F.relu, F.linear, F.batch_norm(training=True) and their
  autograd, here on leaves made once), both on the GPU, us per step between device events around `--reps` back-to-back steps after a warm-up, the two
  alternated three times, median and spread ((max - min) / median) of the three;
* the forward alone and the backward alone of the HIP path, timed the same way;
* the FLOPs of the six matrix products and the achieved FLOP/s of the HIP step -- a whole-step rate that includes the launch
  gaps and the row kernels, not a kernel's share of peak;
* both paths checked against each other on the timed (general) inputs: the largest difference of the logits and of dW2.  At
  16 x 64 x 80 that is 21 M general pre-activations, a handful of which round to the other side of the ReLU kink in one path or
  the other; each such element is worth a whole term of dW2, so this difference says little there;
* both paths against the float64 restatement of the tests, evaluated on the device, in the gates' measure, on the dyadic inputs
  of the tests' sweep (no mask element can flip): `against_float64`.

`--hip-only`: the HIP steps alone, a few of them, for a kernel trace.  The exit status is 0 either way: nobody had measured
either side when this tool was written, and DESIGN.md 7l records what it found."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import ops                                                        # noqa: E402
from tests import head_train_common as H                                        # noqa: E402

SHAPES = ((4, 24, 24), (16, 64, 80))


def gemm_flops(n, dx2):
    return 2 * n * 256 * (256 * (3 if dx2 else 2) + 65 * 3)


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


def accuracy(dev, b, hc, wc):
    """Both paths against the float64 restatement (tests/head_train_common.py: restate64, evaluated on the device) in the
    gates' measure err(T) = max |T - T64| / S_T, on the dyadic inputs of the tests' shape sweep (sweep_case: h is exact in
    float32, so no ReLU mask element can flip by a rounding).  The test suite gates the same at N = 66049 (slices of
    1280 pixels, column blocks of 80 rows, 65 row partials); this is the figure at the size that is timed."""
    x2, p, dlogits, running = H.sweep_case((b, hc, wc), 900 + b)
    x2, dlogits = x2.to(dev), dlogits.to(dev)
    p = {k: v.to(dev) for k, v in p.items()}
    r = H.restate64(x2, p, dlogits, running=tuple(t.to(dev) for t in running))
    want = {k: r[k].cpu() for k in H.GATED}
    rm, rv = running[0].to(dev), running[1].to(dev)
    f = ops.head_train_forward(x2, p["w2"], p["b2"], p["wd"], p["bd"], p["gamma"], p["beta"], want_prob=False, running_mean=rm,
                               running_var=rv)
    g = ops.head_train_backward(dlogits, x2, p["w2"], p["wd"], p["gamma"], f.saved, want_dx2=True)
    got = dict(g._asdict(), logits=f.logits, running_mean=rm, running_var=rv)
    rm32, rv32 = running[0].to(dev), running[1].to(dev)
    logits32, g32 = H.compose_f32(x2, p, dlogits, running=(rm32, rv32))
    got32 = dict(g32, logits=logits32, running_mean=rm32, running_var=rv32)
    return {"inputs": "tests/head_train_common.py: sweep_case (dyadic x2, W2, b2: h exact in float32)",
            "hip_err": {k: float("%.3g" % H.err(got[k], want[k], r["S"][k])) for k in H.GATED},
            "torch_composition_err": {k: float("%.3g" % H.err(got32[k], want[k], r["S"][k])) for k in H.GATED}}


def bench_shape(dev, b, hc, wc, reps, hip_only):
    n = b * hc * wc
    g = torch.Generator(device=dev).manual_seed(n)
    x2 = torch.randn((b, hc, wc, 256), device=dev, generator=g) * 4
    dlogits = torch.randn((b, 65, hc, wc), device=dev, generator=g) / n
    p = {k: v.to(dev) for k, v in H.sweep_params(5).items()}
    p["w2"] = torch.randn((256, 256), device=dev, generator=g) / 16
    rm, rv = torch.zeros(65, device=dev), torch.ones(65, device=dev)
    saved = torch.empty(ops.lib().balf_head_train_saved_bytes(n), dtype=torch.uint8, device=dev)

    def fwd():
        return ops.head_train_forward(x2, p["w2"], p["b2"], p["wd"], p["bd"], p["gamma"], p["beta"], want_prob=False,
                                      running_mean=rm, running_var=rv, saved=saved)

    def bwd(dx2):
        return ops.head_train_backward(dlogits, x2, p["w2"], p["wd"], p["gamma"], saved, want_dx2=dx2)

    out = {"shape": [b, hc, wc], "pixels": n, "repetitions": reps}
    if hip_only:
        for _ in range(reps):
            fwd(), bwd(True)
        torch.cuda.synchronize()
        return out
    for dx2 in (False, True):
        def hip():
            fwd()
            return bwd(dx2)

        leaves = {k: p[k].clone().requires_grad_() for k in H.PARAMS}      # made once: a step pays for no copy
        xc = x2.clone().requires_grad_(dx2)

        def composed():
            for t in list(leaves.values()) + [xc]:
                t.grad = None
            z = F.linear(F.relu(F.linear(xc, leaves["w2"], leaves["b2"])), leaves["wd"], leaves["bd"]).permute(0, 3, 1, 2)
            logits = F.batch_norm(z, rm, rv, leaves["gamma"], leaves["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
            logits.backward(dlogits)
            return logits.detach(), {"dw2": leaves["w2"].grad}

        f, a = fwd(), bwd(dx2)
        logits_c, grads_c = composed()                                     # warm-up of both, and the check
        agree = {"logits_max_abs_diff": float((f.logits - logits_c).abs().max()),
                 "dw2_max_abs_diff": float((a.dw2 - grads_c["dw2"]).abs().max()), "dw2_max_abs": float(grads_c["dw2"].abs().max())}
        del f, a, logits_c, grads_c
        t_hip, t_comp, t_fwd, t_bwd = [], [], [], []
        for _ in range(3):
            t_hip.append(us_per_call(hip, reps))
            t_comp.append(us_per_call(composed, reps))
            t_fwd.append(us_per_call(fwd, reps))
            t_bwd.append(us_per_call(lambda: bwd(dx2), reps))
        sh, sc = stats(t_hip), stats(t_comp)
        key = "with_dx2" if dx2 else "parameters_only"
        out[key] = {"hip": sh, "hip_forward": stats(t_fwd), "hip_backward": stats(t_bwd), "torch_composition": sc,
                    "speedup": round(sc["median_us"] / sh["median_us"], 2), "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]),
                    "gemm_flops": gemm_flops(n, dx2),
                    "hip_achieved_TFLOP_per_s": round(gemm_flops(n, dx2) / (sh["median_us"] * 1e-6) / 1e12, 2), **agree}
        print(json.dumps({key: out[key], "shape": [b, hc, wc]}), flush=True)
    out["against_float64"] = accuracy(dev, b, hc, wc)
    print(json.dumps({"against_float64": out["against_float64"], "shape": [b, hc, wc]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"metric": "training-mode head, forward + backward (balf_head_train_*) vs the float32 torch-op composition under autograd, "
                     "device-event us per step",
           "device": torch.cuda.get_device_name(dev),
           "shapes": [bench_shape(dev, b, hc, wc, args.reps, args.hip_only) for b, hc, wc in SHAPES]}
    if args.out and not args.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
