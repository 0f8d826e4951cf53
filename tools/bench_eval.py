#!/usr/bin/env python3
"""Batched HSequences evaluation against the one-pair loop:
python tools/bench_eval.py [--out FILE] [--calls N] [--core-only] -> one JSON document.

Leg (i), core only: P = 64 pairs of 480x640 with N = 1000 rows (x, y, 1.0, score) per side -- source points at random,
destination points = the source points warped through a random homography near the identity, jittered, a fifth of them
replaced by outliers.  benchmark_test.evaluate.evaluate_pairs (device-event time per call, warmed up) against the loop of
today's one-pair functions (create_common_region_masks -> check_common_points x 2 -> apply_homography_to_points ->
compute_repeatability, wall time), per pair; the results of the two are checked equal.
Leg (ii), end to end: 12 synthetic sequences x 5 pairs at 480x640 (translated crops of a synthetic image), fp16 model,
25 points.  train_utils.check_val_hsequences_repeatability against the reference-style loop (extract_detections of the
source and of the destination per pair, then the one-pair functions), wall time per pair; the five means are checked equal.
--core-only: one warm-up and one timed evaluate_pairs call of leg (i), nothing else (for a rocprofv3 --kernel-trace run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch, pipeline                                            # noqa: E402
from balf_amd.benchmark_test import evaluate, geometry_tools, repeatability_tools as R   # noqa: E402
from balf_amd.model import get_model                                           # noqa: E402
from balf_amd.utils import synth, train_utils                                  # noqa: E402

H, W = 480, 640


def core_inputs(p, n, seed=0):
    rng = np.random.default_rng(seed)
    srcs, dsts, hs = [], [], []
    for _ in range(p):
        hm = np.array([[1.0 + rng.normal(0, 0.03), rng.normal(0, 0.03), rng.normal(0, 12)],
                       [rng.normal(0, 0.03), 1.0 + rng.normal(0, 0.03), rng.normal(0, 12)],
                       [rng.normal(0, 3e-5), rng.normal(0, 3e-5), 1.0]])
        s = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), np.ones(n), rng.uniform(0, 1, n)], axis=1)
        d = geometry_tools.apply_homography_to_points(s, np.linalg.inv(hm))
        d[:, 2] = 1.0
        d[:, :2] += rng.normal(0, 1.5, (n, 2))
        out = rng.random(n) < 0.2
        d[out, 0], d[out, 1] = rng.uniform(0, W - 1, out.sum()), rng.uniform(0, H - 1, out.sum())
        d[:, 0], d[:, 1] = np.clip(d[:, 0], 0, W - 1), np.clip(d[:, 1], 0, H - 1)
        srcs.append(s)
        dsts.append(d)
        hs.append(hm)
    return srcs, dsts, hs


def one_pair(s, d, hm):
    ms, md = geometry_tools.create_common_region_masks(hm, (H, W), (H, W))
    i_s = R.check_common_points(s[:, [1, 0, 2, 3]], ms)
    i_d = R.check_common_points(d[:, [1, 0, 2, 3]], md)
    if i_s.size == 0 or i_d.size == 0:
        return None
    return R.compute_repeatability(s[i_s], geometry_tools.apply_homography_to_points(d[i_d], hm))


def leg_core(dev, calls, core_only):
    p, n = 64, 1000
    srcs, dsts, hs = core_inputs(p, n)
    args = (torch.from_numpy(np.stack(srcs)).to(dev), torch.full((p,), n, dtype=torch.int32, device=dev),
            torch.from_numpy(np.stack(dsts)).to(dev), torch.full((p,), n, dtype=torch.int32, device=dev),
            torch.from_numpy(np.stack(hs)).to(dev), torch.tensor([[H, W, H, W]] * p, dtype=torch.int32, device=dev))
    evaluate.evaluate_pairs(*args)
    torch.cuda.synchronize()
    if core_only:
        r = evaluate.evaluate_pairs(*args)
        torch.cuda.synchronize()
        return {"valid": int(r.valid.sum())}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        r = evaluate.evaluate_pairs(*args)
    b.record()
    b.synchronize()
    batch_ms = a.elapsed_time(b) / calls
    r.rep_single_scale.cpu()                            # (the first strided device-to-host copy loads its kernel)
    t0 = time.perf_counter()
    for _ in range(calls):
        r = evaluate.evaluate_pairs(*args)
        res = r.rep_single_scale.cpu()                  # with the read a caller needs
    batch_read_ms = (time.perf_counter() - t0) * 1e3 / calls
    for k in range(2):
        one_pair(srcs[k], dsts[k], hs[k])               # warm-up
    t0 = time.perf_counter()
    ref = [one_pair(srcs[k], dsts[k], hs[k]) for k in range(p)]
    loop_ms = (time.perf_counter() - t0) * 1e3
    got = {f: getattr(r, f).cpu().numpy() for f in r._fields}
    same = all((ref[k] is None) == (got["valid"][k] == 0) and
               (ref[k] is None or all(np.array_equal(np.float64(ref[k][f]), np.float64(got[f][k]))
                                      for f in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale",
                                                "error_overlap_multi_scale", "possible_matches")))
               for k in range(p))
    del res
    return {"pairs": p, "rows_per_side": n, "image": f"{H}x{W}", "valid_pairs": int(got["valid"].sum()),
            "candidates_single_scale_mean": float(got["candidates_single_scale"].mean()),
            "evaluate_pairs_ms_per_call": round(batch_ms, 4), "evaluate_pairs_us_per_pair": round(batch_ms * 1e3 / p, 3),
            "evaluate_pairs_with_read_ms_per_call": round(batch_read_ms, 4),
            "one_pair_loop_ms": round(loop_ms, 3), "one_pair_loop_us_per_pair": round(loop_ms * 1e3 / p, 3),
            "speedup_per_pair": round(loop_ms / batch_ms, 2), "speedup_per_pair_with_read": round(loop_ms / batch_read_ms, 2),
            "results_equal": bool(same)}


class Loader:
    def __init__(self, n_seq, n_dst=5):
        self.sequences = [f"s{i}" for i in range(n_seq)]
        self._n_dst = n_dst

    def get_sequence_data(self, i):
        g = synth.synthetic_gray_u8(H + 40, W + 40, 100 + i)
        src = synth.gray_to_rgb_norm(g[20:20 + H, 20:20 + W])
        dsts, hs = [], []
        for k in range(self._n_dst):
            dy, dx = 3 * k - 6, 7 - 3 * k
            dsts.append(synth.gray_to_rgb_norm(g[20 + dy:20 + dy + H, 20 + dx:20 + dx + W]))
            hs.append(np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]]))
        return dict(sequence_name=self.sequences[i], im_src_RGB_norm=src, images_dst_RGB_norm=dsts, h_dst_2_src=hs)


class Cached:
    """the loader with its sequences decoded once (image synthesis is not part of either timing)"""

    def __init__(self, loader):
        self.sequences = loader.sequences
        self._d = [loader.get_sequence_data(i) for i in range(len(loader.sequences))]

    def get_sequence_data(self, i):
        return self._d[i]


def reference_loop(loader, m, dev):
    rs = []
    for i in range(len(loader.sequences)):
        sd = loader.get_sequence_data(i)
        for k, im in enumerate(sd["images_dst_RGB_norm"]):
            ps, _ = pipeline.extract_detections(sd["im_src_RGB_norm"], m, dev)
            pd, _ = pipeline.extract_detections(im, m, dev)
            ms, md = geometry_tools.create_common_region_masks(sd["h_dst_2_src"][k], sd["im_src_RGB_norm"].shape, im.shape)
            i_s = R.check_common_points(ps[:, [1, 0, 2, 3]], ms)
            if i_s.size == 0:
                continue
            i_d = R.check_common_points(pd[:, [1, 0, 2, 3]], md)
            if i_d.size == 0:
                continue
            rs.append(R.compute_repeatability(ps[i_s], geometry_tools.apply_homography_to_points(pd[i_d], sd["h_dst_2_src"][k])))
    keys = ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale", "possible_matches")
    return tuple(np.asarray([r[k] for r in rs]).mean() for k in keys)


def leg_end_to_end(dev):
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(20240))
    m.precision = "fp16"
    m = m.eval().to(dev)
    loader = Cached(Loader(12))
    pairs = 12 * 5
    with torch.inference_mode():
        reference_loop(Cached(Loader(1)), m, dev)                               # warm-up
        train_utils.check_val_hsequences_repeatability(Cached(Loader(1)), m, dev, None, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = reference_loop(loader, m, dev)
        loop_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        got = train_utils.check_val_hsequences_repeatability(loader, m, dev, None, 0)
        batch_s = time.perf_counter() - t0
    return {"sequences": 12, "pairs": pairs, "image": f"{H}x{W}", "precision": "fp16", "num_points": 25,
            "driver_ms": round(batch_s * 1e3, 2), "driver_ms_per_pair": round(batch_s * 1e3 / pairs, 3),
            "reference_loop_ms": round(loop_s * 1e3, 2), "reference_loop_ms_per_pair": round(loop_s * 1e3 / pairs, 3),
            "speedup_per_pair": round(loop_s / batch_s, 2),
            "means": [float(v) for v in got], "means_equal": all(np.array_equal(a, b) for a, b in zip(got, ref))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--core-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    core = leg_core(dev, args.calls, args.core_only)
    print(json.dumps(core), flush=True)
    if args.core_only:
        return
    e2e = leg_end_to_end(dev)
    print(json.dumps(e2e), flush=True)
    doc = {"metric": "batched HSequences evaluation vs the one-pair loop", "device": torch.cuda.get_device_name(dev),
           "core": core, "end_to_end": e2e}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
