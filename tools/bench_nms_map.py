#!/usr/bin/env python3
"""Device time of balf_nms_score_map on the detector's own score maps, against balf_greedy_nms on the same maps in
the same process:

    python tools/bench_nms_map.py [--batch 32] [--height 1080] [--width 1920] [--out profiles/nms_map_bench.json]

Legs: ``box`` at the reference's defaults (size 4, iou 0.1, min_prob 0.015: footprint radius 3) and ``greedy`` at dist_thresh 3
(the box leg's radius), 4 (the training loop's) and 15 (the validation's); the yardstick is ``ops.greedy_nms`` (K = 2048, no border)
at the same dist_thresh.  Device events around ``--calls`` calls, three rounds per leg: median, smallest and largest ms per call.
One map also goes through the NumPy oracle of tests/nms_map_common.py: its CPU time, and the GPU maps must equal it bit for bit.
``--trace-only LEG``: a few calls of one leg and nothing else, for a kernel trace from outside."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balf_amd import arch, ops                                         # noqa: E402
from balf_amd.model import get_model                                   # noqa: E402
from balf_amd.utils import synth                                       # noqa: E402

CONF = 0.015
ROUNDS = 3


def score_maps(b, h, w, dev):
    det = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    det.load_state_dict(synth.synthetic_state_dict(20240))
    det.precision = "fp16"
    det = det.eval().to(dev)
    imgs = torch.from_numpy(np.stack([synth.synthetic_gray_u8(h, w, i, blur=5 if i % 2 == 0 else 3) for i in range(b)])).to(dev)
    prob = det.forward_u8(imgs, want_logits=False)["prob"]
    hp, wp = prob.shape[1:]
    top, left = (hp - (h + (h & 1))) // 2, (wp - (w + (w & 1))) // 2
    return prob[:, top:top + h, left:left + w].contiguous()


def timed(fn, calls):
    """ms per call of ``fn``: ROUNDS rounds of ``calls`` calls between device events."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "rounds_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", default=None, metavar="LEG", help="box, or greedy<d>")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prob = score_maps(a.batch, a.height, a.width, dev)
    h, w = a.height, a.width
    legs = {"box": lambda: ops.nms_score_map(prob, "box", conf_thresh=CONF, size=4, iou=0.1)}
    yard = {}
    for d in (3, 4, 15):
        legs[f"greedy{d}"] = lambda d=d: ops.nms_score_map(prob, "greedy", conf_thresh=CONF, dist_thresh=d)
        yard[f"greedy{d}"] = lambda d=d: ops.greedy_nms(prob, 0, 0, h, w, 0, CONF, d, 2048, 0)
    if a.trace_only:
        for _ in range(3):
            legs[a.trace_only]()
        torch.cuda.synchronize()
        return
    res = {"metric": "balf_nms_score_map ms per batch (device events)", "batch": a.batch, "image": f"{w}x{h}", "calls_per_round": a.calls,
           "rounds": ROUNDS, "conf_thresh": CONF, "candidate_fraction": float((prob >= CONF).float().mean()), "legs": {},
           "yardstick_balf_greedy_nms": {}}
    for name, fn in yard.items():
        res["yardstick_balf_greedy_nms"][name] = timed(fn, a.calls)
    for name, fn in legs.items():
        r = timed(fn, a.calls)
        r["kept_per_image"] = float(fn()[1].float().mean())
        against = "greedy3" if name == "box" else name
        r["yardstick"] = against
        r["ratio_to_yardstick"] = r["ms_median"] / res["yardstick_balf_greedy_nms"][against]["ms_median"]
        res["legs"][name] = r
    # one map through the oracle on the CPU: its time, and the GPU's maps against it
    from tests import nms_map_common as M                             # noqa: E402
    one = prob[0].cpu().numpy()
    res["oracle_cpu_s_per_map"], res["equals_oracle"] = {}, {}
    for name, fp in (("box", lambda: M.box_footprint_direct(4, 0.1)), ("greedy4", lambda: M.square_footprint(4)),
                     ("greedy15", lambda: M.square_footprint(15))):
        t0 = time.perf_counter()
        want, n = M.sweep(one, CONF, fp())
        res["oracle_cpu_s_per_map"][name] = time.perf_counter() - t0
        got, cnt = legs[name]()
        res["equals_oracle"][name] = bool(M.same_map(got[0].cpu().numpy(), want) and int(cnt[0]) == n)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    assert all(res["equals_oracle"].values()), res["equals_oracle"]


if __name__ == "__main__":
    main()
