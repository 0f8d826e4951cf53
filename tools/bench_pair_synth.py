#!/usr/bin/env python3
"""Synthesis of the validation's homography image pairs on the GPU (balf_synth_pairs) against what it feeds:
python tools/bench_pair_synth.py [--out FILE] [--reps N] [--kernel-only] -> one JSON document.

64 pairs from 720 x 1280 RGB sources (synthetic photographs), patch 512, top_k 4500, 4500 label points per image, geometry from
dataset_utils.sample_pair_geometry (seeded).
 (1) balf_synth_pairs alone, inputs resident: device events around `--reps` calls after a warm-up, median and spread
     ((max - min) / median); the bytes it must move = the source footprints read once (the bounding boxes of the two windows'
     taps, 3 bytes a pixel) + the label rows + the four outputs written, over the median -> bytes/s, and that as a fraction of
     the plain 1 : 1 copy of this memory system (6.2 TB/s).
 (2) the same 64 pairs by the NumPy restatement of the tests (tests/pair_synth_common.py: the full image warped, then cropped,
     as the reference does) on 16 host processes.  That is NOT cv2 (absent here; cv2 would be faster): it is labelled as what
     it is.  Wall time, min of two runs; the outputs of pair 0 are checked equal to the kernel's.
 (3) the yardstick: train_utils' own chunk of check_val_repeatability for those 64 pairs (forward of both patches in batches of
     16 on the split-f16 model, both evaluation legs, the one read), wall time around a synchronised call; ratio = (1) / (3).
--kernel-only: one warm-up and two balf_synth_pairs calls, nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import random
import sys
import time
from multiprocessing import get_context

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch, ops                                                 # noqa: E402
from balf_amd.datasets import dataset_utils as DU                              # noqa: E402
from balf_amd.datasets.synthetic_pairs import SyntheticPairs                   # noqa: E402
from balf_amd.model import get_model                                           # noqa: E402
from balf_amd.utils import synth, train_utils                                  # noqa: E402
from tests import pair_synth_common as S                                       # noqa: E402

P, H, W, PATCH, TOP_K, N_PTS = 64, 720, 1280, 512, 4500, 4500
N_IMAGES = 8                                                # distinct photographs; pair i uses image i % 8 (a loader's reuse)
HOM = {"perspective": 0.2, "rotation": 25, "scale": 0.1}
COPY_TBPS = 6.2                                             # plain 1 : 1 copy, tools/hbm_bw_probe.py


def make_inputs():
    ims, labels = [], []
    for i in range(N_IMAGES):
        g = synth.synthetic_gray_u8(H, W, 500 + i)
        ims.append(np.ascontiguousarray(np.stack([g, 255 - g, (g.astype(np.int64) * 2 // 3).astype(np.uint8)], axis=2)))
        labels.append(S.make_labels("uniform", N_PTS, (H, W), 900 + i))
    rng = random.Random(17)
    geo = [DU.sample_pair_geometry((H, W, 3), HOM, PATCH, rng) for _ in range(P)]
    return ims, labels, geo


def footprint_bytes(geo):
    """Source bytes a pair must read: the window itself and the bounding box of the destination window's taps (clipped)."""
    total = 0
    for g in geo:
        ys, xs = np.meshgrid([g["win_dst"][0], g["win_dst"][0] + PATCH - 1], [g["win_dst"][1], g["win_dst"][1] + PATCH - 1])
        sx, sy, _, _ = S.source_q5(S.invert3(g["inv_h"]), ys, xs)
        x0, x1 = max(int(sx.min()), 0), min(int(sx.max()) + 1, W - 1)
        y0, y1 = max(int(sy.min()), 0), min(int(sy.max()) + 1, H - 1)
        total += 3 * PATCH * PATCH + 3 * max(0, x1 - x0 + 1) * max(0, y1 - y0 + 1)
    return total


def stats(ts_ms):
    ts = np.asarray(ts_ms)
    med = float(np.median(ts))
    return {"median_ms": round(med, 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4),
            "spread": round(float((ts.max() - ts.min()) / med), 4)}


def _numpy_pair(job):
    im, pts, g = job
    return S.pair_np(im, pts, TOP_K, g["inv_h"], g["win_src"], g["win_dst"], PATCH)[4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--dry", action="store_true", help="inputs and byte counts only (no GPU)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ims, labels, geo = make_inputs()
    if args.dry:
        print(json.dumps({"bytes_read_min": footprint_bytes(geo) + P * N_PTS * 12, "bytes_written": P * 8 * PATCH * PATCH * 4}))
        return
    idx = [i % N_IMAGES for i in range(P)]
    # (2) the NumPy restatement on 16 host processes: BEFORE this process opens the GPU, in freshly started children
    numpy_doc, e = None, None
    if not args.kernel_only:
        jobs = [(ims[idx[i]], labels[idx[i]], geo[i]) for i in range(P)]
        e = S.pair_np(*jobs[0][:2], TOP_K, geo[0]["inv_h"], geo[0]["win_src"], geo[0]["win_dst"], PATCH)
        tn = []
        with get_context("spawn").Pool(16) as pool:
            pool.map(_numpy_pair, jobs[:16], chunksize=1)
            for _ in range(2):
                t0 = time.perf_counter()
                pool.map(_numpy_pair, jobs, chunksize=1)
                tn.append((time.perf_counter() - t0) * 1e3)
        numpy_doc = {"what": "NumPy restatement (full-image warp, then crop) on 16 host processes; NOT cv2, which would be faster",
                     "wall_ms_min_of_2": round(min(tn), 1), "wall_ms_runs": [round(t, 1) for t in tn]}
    loader = SyntheticPairs([ims[i] for i in idx], [labels[i] for i in idx], HOM, PATCH, TOP_K, 17, batch_pairs=P, device=dev)

    def call():
        return loader.synthesise(0, geo)

    out = call()                                            # warm-up: code objects, workspace
    torch.cuda.synchronize()
    if args.kernel_only:
        call(), call()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "dst_max_min": int(loader.last_dst_max.min())}))
        return

    # (1) the synthesis alone.  synthesise() also uploads 64 matrices and windows (a few KB): timed as the loader runs it, and the
    # two kernels alone between events with everything resident
    d = {"inv_h": torch.from_numpy(np.stack([g["inv_h"] for g in geo]).reshape(P, 9)).to(dev),
         "win_src": torch.tensor([g["win_src"] for g in geo], dtype=torch.int32, device=dev),
         "win_dst": torch.tensor([g["win_dst"] for g in geo], dtype=torch.int32, device=dev)}
    bufs = ops.synth_pairs(loader._packed, loader._offsets, loader._sizes, d["inv_h"], d["win_src"], d["win_dst"], loader._pts,
                           loader._pts_off, TOP_K, PATCH)

    def resident():
        ops.synth_pairs(loader._packed, loader._offsets, loader._sizes, d["inv_h"], d["win_src"], d["win_dst"], loader._pts,
                        loader._pts_off, TOP_K, PATCH, out=bufs)

    for _ in range(10):
        resident()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        resident()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    kern = stats(ts)
    tw = []
    for _ in range(max(10, args.reps // 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        tw.append((time.perf_counter() - t0) * 1e3)
    with_upload = stats(tw)
    bytes_out = P * 8 * PATCH * PATCH * 4
    bytes_in = footprint_bytes(geo) + P * N_PTS * 12
    tbps = (bytes_in + bytes_out) / (kern["median_ms"] * 1e-3) / 1e12
    synth_doc = {"balf_synth_pairs_resident_events": kern, "loader_call_with_geometry_upload_wall": with_upload,
                 "bytes_read_min": int(bytes_in), "bytes_written": int(bytes_out), "achieved_TB_per_s": round(tbps, 3),
                 "fraction_of_plain_copy": round(tbps / COPY_TBPS, 3), "plain_copy_TB_per_s": COPY_TBPS,
                 "dst_max_min": int(bufs[4].min()), "repetitions": args.reps}
    print(json.dumps(synth_doc), flush=True)

    got = [t[0].cpu().numpy() for t in bufs[:4]]
    equal = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, e[:4])) and int(bufs[4][0]) == e[4]
    numpy_doc["pair0_equals_kernel"] = bool(equal)
    print(json.dumps(numpy_doc), flush=True)

    # (3) the yardstick: the evaluation chunk these 64 pairs feed
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(20240))
    m.precision = "fp16"
    m = m.eval().to(dev)
    pairs = [(out[0][p], out[1][p], out[5][p]) for p in range(P)]
    te = []
    with torch.inference_mode():
        train_utils._val_chunk(pairs, m, dev, 15, 25, 16)
        torch.cuda.synchronize()
        for _ in range(5):
            t0 = time.perf_counter()
            train_utils._val_chunk(pairs, m, dev, 15, 25, 16)
            torch.cuda.synchronize()
            te.append((time.perf_counter() - t0) * 1e3)
    ev = stats(te)
    doc = {"metric": "synthesis of 64 validation pairs (720x1280 RGB, patch 512, 4500 labels, top_k 4500) vs the evaluation it feeds",
           "device": torch.cuda.get_device_name(dev), "synthesis": synth_doc, "numpy_restatement_16_processes": numpy_doc,
           "check_val_repeatability_chunk_64_pairs_wall": ev,
           "synthesis_over_evaluation": round(kern["median_ms"] / ev["median_ms"], 5),
           "loader_call_over_evaluation": round(with_upload["median_ms"] / ev["median_ms"], 5)}
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    sys.exit(0 if equal else 1)


if __name__ == "__main__":
    main()
