#!/usr/bin/env python3
"""The resize protocol of the HSequences evaluation, batched, against the one-pair loop:
python tools/bench_resize_eval.py [--out FILE] [--reps N] [--core-only] -> one JSON document.

Leg (i), core only: P = 64 pairs, 1000 rows per side at 240x320 already on the device (half of the destination rows are
source rows carried through the pair's homography with noise), keep_k_points 1000, distance_thresh 5.
benchmark_test.evaluate.evaluate_resize_pairs with the one read a caller needs, against the loop of one-pair
compute_resize_repeatability calls and against the float64 NumPy restatement on the host (tests/resize_repeat_common.py: what a
caller without this library has); wall time, `--reps` repetitions of each, median and spread ((max - min) / median); the results
are checked equal in the same run (batched vs loop: bit for bit; vs NumPy: counts equal, localization_err within 1e-9).
Leg (ii), end to end: evaluate_resize_hsequences on a synthetic loader of mixed image sizes (8 sequences x 3 destinations, fp16
model) against the per-pair loop built from ratio_preserving_resize, detect_batch_u8 on one image and
compute_resize_repeatability; the six lists are checked equal.
`faster_beyond_spread`: batched median * (1 + its spread) < loop median * (1 - its spread).
--core-only: one warm-up and one evaluate_resize_pairs call, nothing else (for a rocprofv3 --kernel-trace run)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch                                                      # noqa: E402
from balf_amd.benchmark_test import evaluate, repeatability_tools as RT       # noqa: E402
from balf_amd.datasets import dataset_utils                                    # noqa: E402
from balf_amd.model import get_model                                           # noqa: E402
from balf_amd.pipeline import detect_batch_u8                                  # noqa: E402
from balf_amd.utils import synth                                               # noqa: E402
from tests import resize_repeat_common as R                                    # noqa: E402

SHAPE, K, THRESH = (240, 320), 1000, 5
KEYS = R.KEYS


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3),
            "spread": round(float((ts.max() - ts.min()) / med), 4)}


def verdict(batch, loop):
    return {"speedup": round(loop["median_ms"] / batch["median_ms"], 2),
            "faster_beyond_spread": bool(batch["median_ms"] * (1 + batch["spread"]) < loop["median_ms"] * (1 - loop["spread"]))}


def timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts), out


def core_inputs(p, n):
    rng = np.random.default_rng(41)
    src, dst, hs = np.empty((p, n, 3)), np.empty((p, n, 3)), []
    for i in range(p):
        h = R.scaled_homography(i, SHAPE, SHAPE)
        src[i] = np.stack([rng.uniform(0, SHAPE[0], n), rng.uniform(0, SHAPE[1], n), rng.uniform(0.01, 1, n)], axis=1)
        wc, wr = R.warp_cols_rows(src[i, :, 1], src[i, :, 0], h)
        dst[i] = np.stack([wr + rng.normal(0, 1.5, n), wc + rng.normal(0, 1.5, n), rng.uniform(0.01, 1, n)], axis=1)
        loose = rng.random(n) < 0.5
        dst[i, loose, 0], dst[i, loose, 1] = rng.uniform(0, SHAPE[0], loose.sum()), rng.uniform(0, SHAPE[1], loose.sum())
        hs.append(h)
    return src, dst, np.stack(hs)


def leg_core(dev, reps, core_only):
    p, n = 64, 1000
    src, dst, h = core_inputs(p, n)
    shapes = np.tile(np.asarray(SHAPE + SHAPE, dtype=np.int32), (p, 1))
    src_t, dst_t = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    cnt = torch.full((p,), n, dtype=torch.int32, device=dev)
    h_t, hi_t, sh_t = torch.from_numpy(h).to(dev), torch.from_numpy(np.linalg.inv(h)).to(dev), torch.from_numpy(shapes).to(dev)

    def batched():
        r = evaluate.evaluate_resize_pairs(src_t, cnt, dst_t, cnt, h_t, sh_t, K, THRESH, h_inv=hi_t, order="rcp")
        return torch.stack([t.double() for t in r], dim=1).cpu().numpy()           # one read

    batched()
    if core_only:
        got = batched()
        return {"pairs": p, "mean_repeatability": float(got[:, 0].mean())}

    def loop():
        out = [RT.compute_resize_repeatability(src[i], dst[i], h[i], SHAPE, SHAPE, K, THRESH) for i in range(p)]
        return np.asarray([[float(r[k]) for k in KEYS] for r in out])

    def host():
        out = [R.resize_repeatability_np(src[i], dst[i], h[i], SHAPE, SHAPE, K, THRESH)[0] for i in range(p)]
        return np.asarray([[float(r[k]) for k in KEYS] for r in out])

    loop()
    b, got = timed(batched, reps)
    l, ref = timed(loop, reps)
    c, cpu = timed(host, max(2, reps // 2))
    return {"pairs": p, "rows_per_side": n, "image": "240x320", "keep_k_points": K, "distance_thresh": THRESH, "repetitions": reps,
            "evaluate_resize_pairs_with_read": b, "one_pair_loop": l, "numpy_restatement_on_host": c,
            "evaluate_resize_pairs_us_per_pair": round(b["median_ms"] * 1e3 / p, 2),
            "one_pair_loop_us_per_pair": round(l["median_ms"] * 1e3 / p, 2), **verdict(b, l),
            "speedup_vs_numpy_on_host": round(c["median_ms"] / b["median_ms"], 2),
            "mean_repeatability": float(got[:, 0].mean()), "results_equal": bool(np.array_equal(got, ref)),
            "equal_to_numpy": bool(np.array_equal(got[:, [0, 2, 3, 4, 5]], cpu[:, [0, 2, 3, 4, 5]]) and
                                   np.abs(got[:, 1] - cpu[:, 1]).max() < 1e-9)}


def pair_loop(loader, m, dev, top_k, thr):
    """The protocol from the one-image / one-pair functions."""
    args = types.SimpleNamespace(resize_shape=list(SHAPE))

    def rows_of(img):
        small = dataset_utils.ratio_preserving_resize(img, SHAPE)
        idx, score, count, _ = detect_batch_u8(m, torch.from_numpy(small).to(dev)[None], 15, 15, top_k)
        n = int(count[0])
        i = idx[0, :n].cpu().numpy().astype(np.int64)
        return np.stack([i // SHAPE[1], i % SHAPE[1], score[0, :n].cpu().numpy().astype(np.float64)], axis=1)

    out = {k: [] for k in KEYS}
    for s in range(len(loader.sequences)):
        d = loader.get_sequence_data(s)
        src_rows = rows_of(d['im_src_BGR'])
        for dst, h in zip(d['images_dst_BGR'], d['homographies']):
            hh = dataset_utils.adapt_homography_to_preprocessing(
                {'homography': h, 'shape': np.array(d['im_src_BGR'].shape[:2]), 'warped_shape': np.array(dst.shape[:2])}, args)
            r = RT.compute_resize_repeatability(src_rows, rows_of(dst), hh, SHAPE, SHAPE, keep_k_points=top_k, distance_thresh=thr)
            for k in KEYS:
                out[k].append(float(r[k]))
    return out


def leg_end_to_end(dev, reps):
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(20240))
    m.precision = "fp16"
    m = m.eval().to(dev)
    loader = R.SyntheticSequences(n_sequences=8, n_dst=3)
    with torch.inference_mode():
        evaluate.evaluate_resize_hsequences(loader, m, dev, top_k_points=K, pixel_threshold=THRESH)     # warm-up
        pair_loop(R.SyntheticSequences(n_sequences=1, n_dst=1), m, dev, K, THRESH)
        torch.cuda.synchronize()
        b, got = timed(lambda: evaluate.evaluate_resize_hsequences(loader, m, dev, top_k_points=K, pixel_threshold=THRESH), reps)
        l, ref = timed(lambda: pair_loop(loader, m, dev, K, THRESH), reps)
    n_pairs = len(got["repeatability"])
    return {"sequences": len(loader.sequences), "pairs": n_pairs, "image_sizes": sorted({d['im_src_BGR'].shape[:2] for d in loader.data}),
            "precision": "fp16", "top_k_points": K, "pixel_threshold": THRESH, "repetitions": reps,
            "evaluate_resize_hsequences": b, "one_pair_loop": l,
            "evaluate_resize_hsequences_ms_per_pair": round(b["median_ms"] / n_pairs, 3),
            "one_pair_loop_ms_per_pair": round(l["median_ms"] / n_pairs, 3), **verdict(b, l),
            "mean_repeatability": float(np.mean(got["repeatability"])),
            "results_equal": all(np.array_equal(np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)) for k in KEYS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--core-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    core = leg_core(dev, args.reps, args.core_only)
    print(json.dumps(core), flush=True)
    if args.core_only:
        return
    e2e = leg_end_to_end(dev, args.reps)
    print(json.dumps(e2e), flush=True)
    doc = {"metric": "resize protocol of the HSequences evaluation, batched, vs the one-pair loop",
           "device": torch.cuda.get_device_name(dev), "core": core, "end_to_end": e2e}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ok = core["results_equal"] and e2e["results_equal"] and core["faster_beyond_spread"] and e2e["faster_beyond_spread"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
