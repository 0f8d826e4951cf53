#!/usr/bin/env python3
"""What one wrapper call costs the host:  python tools/bench_wrapper_call.py [--set launcher|hostkit]  -> one JSON line.

--set launcher (the default): three wrappers of `balf_amd.ops` on inputs too small for the kernels to matter.
--set hostkit: the entry points whose host side lays out a workspace and opts in to dynamic LDS: `nms_topk` on a
128 x 128 map at K = 100 (2 KiB of LDS in the select kernel, no opt-in) and K = 5000 (65 KiB, opt-in), `greedy_nms`,
`extract_patches_batch` with two pyramid levels, and one HardNet forward of 512 patches.

Per leg: wall us per call over back-to-back calls with the device drained at the end, five rounds, their median; `host_us` is
the same loop up to, not including, the drain (what the host alone spends when the device keeps up).  To compare two trees or
two libraries (BALF_HIP_LIB), run it with each on one machine."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                    # noqa: E402

from balf_amd import ops                                                        # noqa: E402

ROUNDS = 5


def launcher_legs(dev):
    score = torch.rand((1, 8, 8), device=dev)
    prob = torch.rand((1, 64, 64), device=dev)
    rgb = torch.zeros((2, 2, 3), dtype=torch.uint8, device=dev)
    return 5000, {"window_nms (7 arguments)": lambda: ops.window_nms(score, 1, 3),
                  "rgb_to_gray_u8 (3 arguments)": lambda: ops.rgb_to_gray_u8(rgb),
                  "nms_topk (16 arguments, workspace)": lambda: ops.nms_topk(prob, 0, 0, 64, 64, 4, 5, 16)}


def hostkit_legs(dev):
    from balf_amd.third_party.hardnet.hardnet_pytorch import HardNet
    from balf_amd.utils import synth
    g = torch.Generator(device="cpu").manual_seed(5)
    prob = torch.rand((1, 128, 128), generator=g).to(dev)
    gray = torch.randint(0, 256, (2, 240, 320), generator=g, dtype=torch.uint8).to(dev)
    xy = (torch.rand((2, 64, 2), generator=g) * torch.tensor([319.0, 239.0])).to(dev)
    hn = HardNet()
    hn.load_state_dict(synth.synthetic_hardnet_state_dict(5))
    hn = hn.eval().to(dev)
    patches = synth.synthetic_patches(512, 1).to(dev)

    def hardnet():
        with torch.inference_mode():
            hn(patches)

    return 2000, {"nms_topk 128x128 K=100": lambda: ops.nms_topk(prob, 0, 0, 128, 128, 0, 3, 100),
                  "nms_topk 128x128 K=5000": lambda: ops.nms_topk(prob, 0, 0, 128, 128, 0, 3, 5000),
                  "greedy_nms 128x128 K=512": lambda: ops.greedy_nms(prob, 0, 0, 128, 128, 4, 0.5, 15, 512, 0),
                  "extract_patches_batch 2x240x320, 64 points, scale 64": lambda: ops.extract_patches_batch(gray, xy, None, 64.0),
                  "hardnet forward, 512 patches": hardnet}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("launcher", "hostkit"), default="launcher")
    which = ap.parse_args().set
    calls, legs = (launcher_legs if which == "launcher" else hostkit_legs)(torch.device("cuda:0"))
    out = {}
    for name, fn in legs.items():
        for _ in range(calls * 2 // 5):
            fn()
        torch.cuda.synchronize()
        wall, host = [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            wall.append(round((time.perf_counter() - t0) / calls * 1e6, 3))
            host.append(round((t1 - t0) / calls * 1e6, 3))
        out[name] = {"median_us": sorted(wall)[ROUNDS // 2], "rounds": wall, "host_median_us": sorted(host)[ROUNDS // 2], "host_rounds": host}
    print(json.dumps({"metric": f"wall us per wrapper call, {ROUNDS} rounds of {calls} back-to-back calls ({which} set)",
                      "calls": out}))


if __name__ == "__main__":
    main()
