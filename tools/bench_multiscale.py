#!/usr/bin/env python3
"""Multi-scale extraction (balf_amd/multiscale.py) against the single-scale calls at its level sizes:
python tools/bench_multiscale.py [--out FILE] [--calls N] [--cases 480x640,1080x1920] [--batches 1,16] -> one JSON document.

Per (image size, batch), gray uint8 input, split-f16 forward, default protocol (sqrt 2, 5 pyramid levels, 1 upsampled, 1500
points): device-event wall time per multi-scale call (warmed up); the sum of pipeline.detect_batch_u8 calls at the same level
sizes (each timed the same way, K = that level's share); the pyramid / budgeted top-K / merge kernel time from the library's
profiling slots (a separate call: the event pairs add their own cost) with its share of the call; the pyramid kernels' bytes
over their time against 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import arch, multiscale as MS, ops, pipeline       # noqa: E402
from balf_amd.model import get_model                              # noqa: E402
from balf_amd.utils import synth                                  # noqa: E402

HBM_TBS = 8.0


def timed(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def pyramid_bytes(plan, b):
    """HBM bytes the pyramid kernels move at the least: each source read once, each padded level written once (gray)."""
    u = plan.upsampled_levels
    h, w = plan.shapes[u]
    total = b * h * w                                               # level U from the uint8 image
    for i, (hp, wp, _, _) in enumerate(plan.padded):
        total += b * 3 * hp * wp * 4                                # the padded three-plane level
        if i != u:
            src = plan.shapes[u] if i < u else plan.shapes[i - 1]
            total += b * src[0] * src[1] * 4                        # one plane of the source level
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default="480x640,1080x1920")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--multiscale-only", action="store_true",
                    help="one warm-up and one multi-scale call per case, nothing else (for a rocprofv3 --kernel-trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(20240))
    m.precision = "fp16"
    m = m.eval().to(dev)
    rows = []
    for case in args.cases.split(","):
        h, w = map(int, case.split("x"))
        plan = MS.pyramid_plan(h, w)
        for b in map(int, args.batches.split(",")):
            imgs = torch.from_numpy(np.stack([synth.synthetic_gray_u8(h, w, i) for i in range(b)])).to(dev)
            if args.multiscale_only:
                with torch.inference_mode():
                    for _ in range(2):
                        MS.detect_batch_multiscale_u8(m, imgs)
                torch.cuda.synchronize()
                continue
            with torch.inference_mode():
                ms_call = timed(lambda: MS.detect_batch_multiscale_u8(m, imgs), args.calls)
                single = []
                for i, (hh, ww) in enumerate(plan.shapes):
                    li = torch.from_numpy(np.stack([synth.synthetic_gray_u8(hh, ww, j) for j in range(b)])).to(dev)
                    k = max(1, plan.point_level[i])
                    single.append(timed(lambda: pipeline.detect_batch_u8(m, li, 15, 15, k), args.calls))
                    del li
                torch.cuda.synchronize()
                ops.profile_begin()
                MS.detect_batch_multiscale_u8(m, imgs)
                torch.cuda.synchronize()
                prof = ops.profile_end()
            slot = lambda name: prof.get(name, (0.0, 0))[0]
            pyr, merge = slot("ms_pyramid"), slot("ms_merge")
            budget = slot("nms_tile") + slot("topk_select")
            prof_total = sum(v[0] for v in prof.values())
            nbytes = pyramid_bytes(plan, b)
            rows.append({
                "image": f"{h}x{w}", "batch": b, "levels": [f"{hh}x{ww}" for hh, ww in plan.shapes],
                "multiscale_ms_per_call": round(ms_call, 4),
                "single_scale_ms_sum": round(sum(single), 4),
                "single_scale_ms_by_level": [round(v, 4) for v in single],
                "ratio_to_single_scale_sum": round(ms_call / sum(single), 4),
                "kernel_ms": {"pyramid": round(pyr, 4), "budget_topk": round(budget, 4), "merge": round(merge, 4),
                              "all_profiled": round(prof_total, 4)},
                "kernel_share_of_profiled_call": {"pyramid": round(pyr / prof_total, 4),
                                                  "budget_topk": round(budget / prof_total, 4),
                                                  "merge": round(merge / prof_total, 4)},
                "pyramid_launches": prof.get("ms_pyramid", (0, 0))[1],
                "pyramid_bytes": nbytes,
                "pyramid_tb_per_s": round(nbytes / (pyr * 1e-3) / 1e12, 3) if pyr > 0 else None,
                "pyramid_fraction_of_8tbs": round(nbytes / (pyr * 1e-3) / 1e12 / HBM_TBS, 3) if pyr > 0 else None,
            })
            print(json.dumps(rows[-1]), flush=True)
            del imgs
            ops.release_workspaces()
            torch.cuda.empty_cache()
    doc = {"metric": "multi-scale extraction vs single-scale calls at its level sizes", "precision": "fp16",
           "input": "gray uint8", "protocol": "sqrt(2), 5 pyramid levels, 1 upsampled, 1500 points, nms 15, border 15",
           "device": torch.cuda.get_device_name(dev), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
