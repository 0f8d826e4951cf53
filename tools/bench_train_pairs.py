#!/usr/bin/env python3
"""Synthesis of the TRAINING task's image pairs (balf_synth_train_pairs) against its two-call composition and the validation
task's balf_synth_pairs:  python tools/bench_train_pairs.py [--out FILE] [--reps N] [--plain-only | --kernel-only]
-> one JSON document.

The workload of tools/bench_pair_synth.py: 64 pairs from 720 x 1280 RGB sources, patch 512, top_k 4500, 4500 label points per
image, seeded geometry; the photometric parameters are 64 seeded sample_photometric draws.  Everything is resident; each figure
is the median of THREE rounds of `--reps` calls between device events (a round's value is its median), with the spread
(max - min) / median over the rounds and the rounds themselves:
 (1) balf_synth_train_pairs: two launches, the distortion applied to the taps of the destination window only;
 (2) the composition: balf_photometric_u8 over the 64 whole source images (64 x 2.76 MB read and written), then balf_synth_pairs
     on its output -- the same destination patch, heat maps and dst_max, bit for bit (checked here and in
     tests/test_photometric_gpu.py; its source patch is cut from the distorted image, which is not the training task's);
 (3) balf_synth_pairs alone: the validation task, what (1) adds the distortion to.
The label kernel is the same code in (1) and (3), so (1) - (3) is the difference of the image kernel's two forms.
--plain-only: (3) alone, through nothing newer than ops.synth_pairs: the same script measures an older tree's library.
--kernel-only: one warm-up and two calls of each entry, nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_pair_synth as B                                                   # noqa: E402
from balf_amd import ops                                                       # noqa: E402
from balf_amd.datasets import dataset_utils as DU                              # noqa: E402
from balf_amd.datasets.synthetic_pairs import SyntheticPairs                   # noqa: E402

ROUNDS = 3


def rounds(fn, reps):
    meds = []
    for _ in range(ROUNDS):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        meds.append(float(np.median(ts)))
    med = float(np.median(meds))
    return {"median_ms": round(med, 4), "rounds_ms": [round(m, 4) for m in meds], "spread": round((max(meds) - min(meds)) / med, 4),
            "repetitions_per_round": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P, PATCH, TOP_K = B.P, B.PATCH, B.TOP_K
    ims, labels, geo = B.make_inputs()
    idx = [i % B.N_IMAGES for i in range(P)]
    loader = SyntheticPairs([ims[i] for i in idx], [labels[i] for i in idx], B.HOM, PATCH, TOP_K, 17, batch_pairs=P, device=dev)
    inv_h = torch.from_numpy(np.stack([g["inv_h"] for g in geo]).reshape(P, 9)).to(dev)
    win_src = torch.tensor([g["win_src"] for g in geo], dtype=torch.int32, device=dev)
    win_dst = torch.tensor([g["win_dst"] for g in geo], dtype=torch.int32, device=dev)
    common = (loader._offsets, loader._sizes, inv_h, win_src, win_dst, loader._pts, loader._pts_off, TOP_K, PATCH)
    bufs = ops.synth_pairs(loader._packed, *common)

    def plain():
        ops.synth_pairs(loader._packed, *common, out=bufs)

    doc = {"metric": "64 pairs (720x1280 RGB, patch 512, 4500 labels, top_k 4500), everything resident, device events",
           "device": torch.cuda.get_device_name(dev)}
    if not args.plain_only:
        prng = np.random.RandomState(17)
        sets = [DU.sample_photometric(prng) for _ in range(P)]
        params = torch.from_numpy(np.stack([s["params"] for s in sets])).to(dev)
        perm = torch.tensor([s["perm"] for s in sets], dtype=torch.int32, device=dev)
        distorted = torch.empty_like(loader._packed)
        bufs2 = tuple(torch.empty_like(t) for t in bufs)

        def fused():
            ops.synth_train_pairs(loader._packed, *common, params, perm, out=bufs)

        def composed():
            ops.photometric_u8(loader._packed, loader._offsets, loader._sizes, params, perm, 2, out=distorted)
            ops.synth_pairs(distorted, *common, out=bufs2)

        fused(), composed()
        torch.cuda.synchronize()
        equal = all(torch.equal(a, b) for a, b in zip(bufs[1:], bufs2[1:]))     # (the composition's SOURCE patch is distorted too)
        if args.kernel_only:
            for _ in range(2):
                fused(), composed()
            torch.cuda.synchronize()
            print(json.dumps({"kernel_only": True, "fused_equals_composition": equal}))
            return
        doc["synth_train_pairs"] = rounds(fused, args.reps)
        doc["photometric_u8_then_synth_pairs"] = rounds(composed, args.reps)
        doc["fused_equals_composition"] = equal
        doc["whole_image_bytes_read_and_written_by_the_composition"] = 2 * int(loader._packed.numel())
    doc["synth_pairs"] = rounds(plain, args.reps)
    if not args.plain_only:
        doc["train_minus_plain_ms"] = round(doc["synth_train_pairs"]["median_ms"] - doc["synth_pairs"]["median_ms"], 4)
        doc["composition_over_fused"] = round(doc["photometric_u8_then_synth_pairs"]["median_ms"] / doc["synth_train_pairs"]["median_ms"], 3)
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    sys.exit(0 if doc.get("fused_equals_composition", True) else 1)


if __name__ == "__main__":
    main()
