#!/usr/bin/env python3
"""Batched synthetic-pair validation (check_val_repeatability) against the one-pair loop:
python tools/bench_val.py [--out FILE] [--reps N] [--core-only LEG] -> one JSON document.

Leg (i), core only: P = 64 pairs of 256x320 score maps already on the device (the fp16 model's score maps of synthetic
images; the destination is a translated crop of the same scene, so the homography is a known translation), num_points 25,
nms_size 15.  benchmark_test.evaluate.evaluate_val_pairs, BOTH legs (greedy + window) per repetition, with the one read a
caller needs, against the loop over the pairs built from the one-pair functions that existed before it
(test_utils.apply_nms, ops.greedy_nms + scatter, geometry_tools.create_common_region_masks, get_point_coordinates,
apply_homography_to_points, compute_repeatability); wall time, `--reps` repetitions of each, median and spread
((max - min) / median); the results of the two are checked equal in the same run.
Leg (ii), end to end: train_utils.check_val_repeatability on a synthetic loader (32 batches of 2 pairs at 256x320, fp16
model) against the same loop with one forward per image of element 0; the ten values are checked equal.
`faster_beyond_spread`: batched median * (1 + its spread) < loop median * (1 - its spread).
--core-only LEG: one warm-up and one evaluate_val_pairs call of that leg, nothing else (for a rocprofv3 --kernel-trace run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch, ops                                                 # noqa: E402
from balf_amd.benchmark_test import evaluate, geometry_tools, repeatability_tools as R   # noqa: E402
from balf_amd.model import get_model                                           # noqa: E402
from balf_amd.utils import synth, test_utils, train_utils                      # noqa: E402

H, W, NMS, K, CONF = 256, 320, 15, 25, 0.015
KEYS = ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale", "possible_matches")


def pair_images(i):
    """-> (src [3,H,W], dst [3,H,W] float32, h_dst_2_src): two crops of one synthetic scene, a known translation apart."""
    g = synth.synthetic_gray_u8(H + 40, W + 40, 300 + i)
    dy, dx = (i % 7) - 3, 4 - (i % 9)
    src = torch.from_numpy(g[20:20 + H, 20:20 + W].astype(np.float32) / 255.0)
    dst = torch.from_numpy(g[20 + dy:20 + dy + H, 20 + dx:20 + dx + W].astype(np.float32) / 255.0)
    h = np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])
    return src[None].expand(3, -1, -1).contiguous(), dst[None].expand(3, -1, -1).contiguous(), h


def one_pair(prob_src, prob_dst, h, leg):
    """The per-pair body of the reference's loop from the one-pair functions; ``prob_*``: [H,W] float32 NumPy."""
    ms, md = geometry_tools.create_common_region_masks(h, prob_src.shape, prob_dst.shape)
    rows = []
    for prob, mask in ((prob_src, ms), (prob_dst, md)):
        if leg == "window":
            nms = test_utils.apply_nms(prob, NMS)
        else:
            t = torch.from_numpy(prob).cuda().unsqueeze(0)
            idx, score, _, count, _ = ops.greedy_nms(t, 0, 0, H, W, 0, CONF, NMS, 1024, 0)
            n = int(count[0])
            nms = np.zeros_like(prob)
            nms.ravel()[idx[0, :n].cpu().numpy().astype(np.int64)] = score[0, :n].cpu().numpy()
        rows.append(test_utils.get_point_coordinates(np.multiply(nms, mask), num_points=K, order_coord='xysr'))
    return R.compute_repeatability(rows[0], geometry_tools.apply_homography_to_points(rows[1], h))


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3),
            "spread": round(float((ts.max() - ts.min()) / med), 4)}


def verdict(batch, loop):
    return {"speedup": round(loop["median_ms"] / batch["median_ms"], 2),
            "faster_beyond_spread": bool(batch["median_ms"] * (1 + batch["spread"]) < loop["median_ms"] * (1 - loop["spread"]))}


def load_model(dev):
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(20240))
    m.precision = "fp16"
    return m.eval().to(dev)


def leg_core(dev, m, reps, core_only):
    p = 64
    ims = [pair_images(i) for i in range(p)]
    with torch.inference_mode():
        ps = torch.cat([m(torch.stack([im[0] for im in ims[b:b + 16]]).to(dev), want_logits=False)["prob"] for b in range(0, p, 16)])
        pd = torch.cat([m(torch.stack([im[1] for im in ims[b:b + 16]]).to(dev), want_logits=False)["prob"] for b in range(0, p, 16)])
    hh = torch.from_numpy(np.stack([im[2] for im in ims])).to(dev)
    torch.cuda.synchronize()

    def batched():
        out = [evaluate.evaluate_val_pairs(ps, pd, hh, NMS, K, leg=leg, conf_thresh=CONF) for leg in ("greedy", "window")]
        return torch.stack([torch.stack([getattr(r, k).double() for k in KEYS], dim=1) for r in out]).cpu().numpy()   # one read

    batched()
    if core_only:
        r = evaluate.evaluate_val_pairs(ps, pd, hh, NMS, K, leg=core_only, conf_thresh=CONF)
        torch.cuda.synchronize()
        return {"leg": core_only, "rows": int(r.kept.sum())}
    tb = []
    with torch.inference_mode():
        for _ in range(reps):
            t0 = time.perf_counter()
            got = batched()
            tb.append(time.perf_counter() - t0)
    ps_h, pd_h, hs = ps.cpu().numpy(), pd.cpu().numpy(), [im[2] for im in ims]

    def loop():
        return np.asarray([[[float(one_pair(ps_h[k], pd_h[k], hs[k], leg)[f]) for f in KEYS] for k in range(p)]
                           for leg in ("greedy", "window")])

    one_pair(ps_h[0], pd_h[0], hs[0], "greedy"), one_pair(ps_h[0], pd_h[0], hs[0], "window")          # warm-up
    tl = []
    with torch.inference_mode():
        for _ in range(reps):
            t0 = time.perf_counter()
            ref = loop()
            tl.append(time.perf_counter() - t0)
    b, l = stats(tb), stats(tl)
    return {"pairs": p, "maps": f"{H}x{W}", "num_points": K, "nms_size": NMS, "legs": "greedy + window", "repetitions": reps,
            "evaluate_val_pairs_both_legs_with_read": b, "one_pair_loop_both_legs": l,
            "evaluate_val_pairs_us_per_pair_leg": round(b["median_ms"] * 1e3 / (2 * p), 2),
            "one_pair_loop_us_per_pair_leg": round(l["median_ms"] * 1e3 / (2 * p), 2), **verdict(b, l),
            "mean_rep_single_scale": [float(got[0, :, 0].mean()), float(got[1, :, 0].mean())],
            "results_equal": bool(np.array_equal(got, ref, equal_nan=True))}


def make_loader(n):
    out = []
    for i in range(n):
        a, b = pair_images(2 * i), pair_images(2 * i + 1)
        hh = torch.from_numpy(np.stack([a[2], b[2]]))
        z = torch.zeros((2, 1, H, W))
        out.append((torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]]), z, z, torch.linalg.inv(hh), hh))
    return out


def reference_loop(loader, m, dev):
    """The reference's loop with one forward per image of element 0 and the one-pair functions."""
    greedy, last = [], None
    for batch in loader:
        ps = m(batch[0][:1].to(dev), want_logits=False)["prob"][0].cpu().numpy()
        pd = m(batch[1][:1].to(dev), want_logits=False)["prob"][0].cpu().numpy()
        h = batch[5][0].numpy()
        r = one_pair(ps, pd, h, "greedy")
        greedy.append([float(r[f]) for f in KEYS])
        r = one_pair(ps, pd, h, "window")
        last = [float(r[f]) for f in KEYS]
    g = np.ascontiguousarray(np.asarray(greedy).T)
    return tuple(g[i].mean() for i in range(5)) + tuple(last)


def leg_end_to_end(dev, m, reps):
    n = 32
    loader = make_loader(n)
    with torch.inference_mode():
        reference_loop(loader[:1], m, dev)                                      # warm-up
        train_utils.check_val_repeatability(loader[:2], m, dev, None, 0)
        torch.cuda.synchronize()
        tb, tl = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = train_utils.check_val_repeatability(loader, m, dev, None, 0)
            tb.append(time.perf_counter() - t0)
        for _ in range(reps):
            t0 = time.perf_counter()
            ref = reference_loop(loader, m, dev)
            tl.append(time.perf_counter() - t0)
    b, l = stats(tb), stats(tl)
    return {"loader_batches": n, "batch_size": 2, "image": f"{H}x{W}", "precision": "fp16", "num_points": K, "repetitions": reps,
            "check_val_repeatability": b, "reference_loop": l,
            "check_val_repeatability_ms_per_pair": round(b["median_ms"] / n, 3),
            "reference_loop_ms_per_pair": round(l["median_ms"] / n, 3), **verdict(b, l),
            "ten": [float(v) for v in got],
            "results_equal": all(np.array_equal(np.float64(a), np.float64(c)) for a, c in zip(got, ref))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--core-only", choices=("greedy", "window"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = load_model(dev)
    core = leg_core(dev, m, args.reps, args.core_only)
    print(json.dumps(core), flush=True)
    if args.core_only:
        return
    e2e = leg_end_to_end(dev, m, args.reps)
    print(json.dumps(e2e), flush=True)
    doc = {"metric": "batched synthetic-pair validation (check_val_repeatability) vs the one-pair loop",
           "device": torch.cuda.get_device_name(dev), "core": core, "end_to_end": e2e}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ok = core["results_equal"] and e2e["results_equal"] and core["faster_beyond_spread"] and e2e["faster_beyond_spread"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
