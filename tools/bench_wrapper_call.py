#!/usr/bin/env python3
"""What one wrapper call costs the host:  python tools/bench_wrapper_call.py  -> one JSON line.

Three wrappers of `balf_amd.ops` on inputs too small for the kernels to matter: wall us per call over 5000 back-to-back calls with
the device drained at the end, five rounds, their median.  To compare two trees, run it in each on the same library."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                    # noqa: E402

from balf_amd import ops                                                        # noqa: E402

CALLS, ROUNDS = 5000, 5


def main():
    dev = torch.device("cuda:0")
    score = torch.rand((1, 8, 8), device=dev)
    prob = torch.rand((1, 64, 64), device=dev)
    rgb = torch.zeros((2, 2, 3), dtype=torch.uint8, device=dev)
    legs = {"window_nms (7 arguments)": lambda: ops.window_nms(score, 1, 3),
            "rgb_to_gray_u8 (3 arguments)": lambda: ops.rgb_to_gray_u8(rgb),
            "nms_topk (16 arguments, workspace)": lambda: ops.nms_topk(prob, 0, 0, 64, 64, 4, 5, 16)}
    out = {}
    for name, fn in legs.items():
        for _ in range(2000):
            fn()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            rounds.append(round((time.perf_counter() - t0) / CALLS * 1e6, 3))
        out[name] = {"median_us": sorted(rounds)[ROUNDS // 2], "rounds": rounds}
    print(json.dumps({"metric": f"wall us per wrapper call, {ROUNDS} rounds of {CALLS} back-to-back calls, tiny inputs (host-bound)",
                      "calls": out}))


if __name__ == "__main__":
    main()
