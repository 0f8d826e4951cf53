#!/usr/bin/env python3
"""Stage 4's channel-attention block plus the head in training mode (forward + backward) on the GPU against the torch-op
composition: python tools/bench_tail_train.py [--out FILE] [--reps N] [--hip-only] -> one JSON document.

Shapes: 4 x 24 x 24 (the reference's training batch: four 192-pixel patches) and 16 x 64 x 80 (sixteen VGA images), as
(B, Hc, Wc) of the stage-4 features [B,Hc,Wc,256].  Per shape:

* one training step of the tail through the library -- `ops.rcab_train_forward`, `ops.head_train_forward`, then
  `ops.head_train_backward` with dx2 and `ops.rcab_train_backward` (6 + 5 + 13 + 16 launches; prob not requested, running
  statistics updated, dy requested or not) -- and the same step by the float32 torch-op composition the tests state
  (tests/rcab_train_common.py: F.layer_norm, F.linear, F.leaky_relu, mean, sigmoid; then tests/head_train_common.py's F.linear,
  F.relu, F.linear, F.batch_norm(training=True)) under autograd, on leaves made once.  Both on the GPU, us per step between
  device events around `--reps` back-to-back steps after a warm-up, the two alternated three times, median and spread ((max -
  min) / median) of the three;
* the four library calls alone, timed the same way;
* the FLOPs of the twelve matrix products and the achieved FLOP/s of the HIP step -- a whole-step rate that includes the launch
  gaps and the row kernels, not a kernel's share of peak;
* both paths checked against each other on the timed (general) inputs: the largest difference of the logits and of dwc1 (a
  handful of the general pre-activations round to the other side of a kink in one path or the other, each worth a whole term);
* the block's twelve outputs of both paths against the float64 restatement of the tests, evaluated on the device, in the
  gates' measure, on the inputs of the tests' sweep (no pre-activation within 1e-3 of a kink): `against_float64`.  The suite
  gates the same at (2, 257, 257), the smallest shape with row blocks of more than 64 rows; this is the figure at
  the size that is timed.

`--hip-only`: the HIP steps alone, a few of them, for a kernel trace.  The exit status is 0 either way: nobody had measured
either side when this tool was written, and DESIGN.md 7m records what it found."""
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
from tests import rcab_train_common as R                                        # noqa: E402

SHAPES = ((4, 24, 24), (16, 64, 80))


def gemm_flops(n, dy):
    return 2 * n * 256 * (256 * (5 if dy else 4) + 256 * 3 + 65 * 3)           # the block's, the head's with dx2


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
    """The block's outputs of both paths against restate64 (evaluated on the device) in the gates' measure err(T) = max |T - T64|
    / S_T, on the inputs of the tests' shape sweep (sweep_case: no h and no SE pre-activation within 1e-3 of 0)."""
    y, r, p, g = (t.to(dev) if isinstance(t, torch.Tensor) else {k: v.to(dev) for k, v in t.items()}
                  for t in R.sweep_case((b, hc, wc), 900 + b))
    res = R.restate64(y, r, p, g)
    want = {k: res[k].cpu() for k in R.GATED}
    params = [p[k] for k in R.PARAMS]
    f = ops.rcab_train_forward(y, r, params)
    back = ops.rcab_train_backward(g, y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], f.saved, want_dy=True)
    got = dict(back._asdict(), x2=f.x2)
    x2_32, g32 = R.compose_f32(y, r, p, g)
    got32 = dict(g32, x2=x2_32)
    return {"inputs": "tests/rcab_train_common.py: sweep_case (rows within 1e-3 of the LeakyReLU kink redrawn)",
            "hip_err": {k: float("%.3g" % R.err(got[k], want[k], res["S"][k])) for k in R.GATED},
            "torch_composition_err": {k: float("%.3g" % R.err(got32[k], want[k], res["S"][k])) for k in R.GATED}}


def bench_shape(dev, b, hc, wc, reps, hip_only):
    n = b * hc * wc
    g = torch.Generator(device=dev).manual_seed(n)
    y = torch.randn((b, hc, wc, 256), device=dev, generator=g) * 2
    r = y + torch.randn((b, hc, wc, 256), device=dev, generator=g).clamp(min=0)
    dlogits = torch.randn((b, 65, hc, wc), device=dev, generator=g) / n
    p = {k: v.to(dev) for k, v in R.sweep_params(5)[0].items()}
    hp = {k: v.to(dev) for k, v in H.sweep_params(5).items()}
    hp["w2"] = torch.randn((256, 256), device=dev, generator=g) / 16
    params = [p[k] for k in R.PARAMS]
    rm, rv = torch.zeros(65, device=dev), torch.ones(65, device=dev)
    saved_r = torch.empty(ops.lib().balf_rcab_train_saved_bytes(b, hc, wc), dtype=torch.uint8, device=dev)
    saved_h = torch.empty(ops.lib().balf_head_train_saved_bytes(n), dtype=torch.uint8, device=dev)
    state = {}

    def rcab_fwd():
        state["x2"] = ops.rcab_train_forward(y, r, params, saved=saved_r).x2

    def head_fwd():
        return ops.head_train_forward(state["x2"], hp["w2"], hp["b2"], hp["wd"], hp["bd"], hp["gamma"], hp["beta"], want_prob=False,
                                      running_mean=rm, running_var=rv, saved=saved_h)

    def head_bwd():
        state["dx2"] = ops.head_train_backward(dlogits, state["x2"], hp["w2"], hp["wd"], hp["gamma"], saved_h, want_dx2=True).dx2

    def rcab_bwd(dy):
        return ops.rcab_train_backward(state["dx2"], y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], saved_r, want_dy=dy)

    def hip(dy):
        rcab_fwd()
        f = head_fwd()
        head_bwd()
        return f, rcab_bwd(dy)

    out = {"shape": [b, hc, wc], "pixels": n, "repetitions": reps}
    if hip_only:
        for _ in range(reps):
            hip(True)
        torch.cuda.synchronize()
        return out
    for dy in (False, True):
        leaves = {k: p[k].clone().requires_grad_() for k in R.PARAMS}      # made once: a step pays for no copy
        hl = {k: hp[k].clone().requires_grad_() for k in H.PARAMS}
        yc = y.clone().requires_grad_(dy)
        x0 = r - y

        def composed():
            for t in list(leaves.values()) + list(hl.values()) + [yc]:
                t.grad = None
            nrm = F.layer_norm(yc, (256,), leaves["ln_g"], leaves["ln_b"], R.LN_EPS)
            t = F.linear(F.leaky_relu(F.linear(nrm, leaves["wc1"], leaves["bc1"]), R.SLOPE), leaves["wc2"], leaves["bc2"])
            s = torch.sigmoid(F.linear(F.relu(F.linear(t.mean(dim=(1, 2)), leaves["ws0"], leaves["bs0"])), leaves["ws2"],
                                       leaves["bs2"]))
            x2 = t * s[:, None, None, :] + yc + x0
            z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
            logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
            logits.backward(dlogits)
            return logits.detach(), leaves["wc1"].grad

        f, a = hip(dy)
        logits_c, dwc1_c = composed()                                      # warm-up of both, and the check
        agree = {"logits_max_abs_diff": float((f.logits - logits_c).abs().max()),
                 "dwc1_max_abs_diff": float((a.dwc1 - dwc1_c).abs().max()), "dwc1_max_abs": float(dwc1_c.abs().max())}
        del f, a, logits_c, dwc1_c
        times = {k: [] for k in ("hip", "torch_composition", "rcab_forward", "head_forward", "head_backward", "rcab_backward")}
        for _ in range(3):
            times["hip"].append(us_per_call(lambda: hip(dy), reps))
            times["torch_composition"].append(us_per_call(composed, reps))
            times["rcab_forward"].append(us_per_call(rcab_fwd, reps))
            times["head_forward"].append(us_per_call(head_fwd, reps))
            times["head_backward"].append(us_per_call(head_bwd, reps))
            times["rcab_backward"].append(us_per_call(lambda: rcab_bwd(dy), reps))
        st = {k: stats(v) for k, v in times.items()}
        sh, sc = st["hip"], st["torch_composition"]
        key = "with_dy" if dy else "parameters_only"
        out[key] = {**st, "speedup": round(sc["median_us"] / sh["median_us"], 2),
                    "hip_not_slower": bool(sh["median_us"] <= sc["median_us"]), "gemm_flops": gemm_flops(n, dy),
                    "hip_achieved_TFLOP_per_s": round(gemm_flops(n, dy) / (sh["median_us"] * 1e-6) / 1e12, 2), **agree}
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
    doc = {"metric": "stage 4's RCAB + the head in training mode, forward + backward (balf_rcab_train_* + balf_head_train_*) vs the "
                     "float32 torch-op composition under autograd, device-event us per step",
           "device": torch.cuda.get_device_name(dev),
           "shapes": [bench_shape(dev, b, hc, wc, args.reps, args.hip_only) for b, hc, wc in SHAPES]}
    if args.out and not args.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
