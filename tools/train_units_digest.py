#!/usr/bin/env python3
"""sha256 of every output tensor of the four training units (head, rcab, gmlp, linrelu), forward and backward, on seeded inputs:
`sha256  unit shape case: tensor`, one line per tensor, then one line over all of them.  Two libraries whose listings are equal
compute the same bits at these shapes: run it once per library (BALF_HIP_LIB names the one to load) and compare.

    python tools/train_units_digest.py [--out FILE]

The inputs are the sweep cases of tests/*_train_common.py, drawn on the CPU generator.  The shapes are the rows of
tests/train_common.py: GUARD_SHAPES that reach each regime of the LayerNorm and column-sum kernels: one block and several, a ragged
last block, two slabs, and the col_rows > 64 regime.  The RCAB's backward runs without dy, with dy, and with dx2 and dy 4 bytes
behind a 16-byte boundary (the 4-byte path of ld4 / st4); the gMLP's without and with dx0."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import _lib, ops                                                  # noqa: E402
from tests import gmlp_train_common as G                                        # noqa: E402
from tests import head_train_common as H                                        # noqa: E402
from tests import linrelu_train_common as L                                     # noqa: E402
from tests import rcab_train_common as R                                        # noqa: E402

SHAPES = {
    "rcab": ((2, 1, 1), (1, 5, 13), (2, 7, 9), (1, 1, 257), (1, 129, 131), (2, 257, 257)),
    "gmlp": ((1, 8, 8), (2, 8, 16), (1, 8, 40), (1, 8, 2056), (2, 216, 152)),
    "head": ((1, 1, 2), (1, 5, 13), (1, 1, 257)),
    "linrelu": ((65, 32), (257, 64)),
}
SEED = 7


def off4(t):
    """A contiguous tensor of t's shape and values that starts 4 bytes behind a 16-byte boundary."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def rcab(shape, dev):
    y, r, p, dx2 = R.sweep_case(shape, SEED, device=dev)
    params = [p[k] for k in R.PARAMS]
    fwd = ops.rcab_train_forward(y, r, params)
    yield "forward", {"x2": fwd.x2}
    reads = [p[k] for k in ops._RCAB_BACKWARD_READS]
    names = ["d" + k for k in R.PARAMS]
    back = ops.rcab_train_backward(dx2, y, *reads, fwd.saved, want_dy=False)
    yield "backward", dict(zip(names, back[:10]))
    back = ops.rcab_train_backward(dx2, y, *reads, fwd.saved, want_dy=True)
    yield "backward dy", dict(zip(names + ["dy"], back))
    back = ops.rcab_train_backward(off4(dx2), y, *reads, fwd.saved, want_dy=off4(torch.zeros_like(y)))
    yield "backward dy, dx2 and dy 4 bytes off", dict(zip(names + ["dy"], back))


def gmlp(shape, dev):
    x0, p, dy = G.sweep_case(shape, SEED, device=dev)
    params = [p[k] for k in G.PARAMS]
    fwd = ops.gmlp_train_forward(x0, params)
    yield "forward", {"y": fwd.y}
    names = ["d:" + k for k in G.PARAMS]
    back = ops.gmlp_train_backward(dy, x0, params, fwd.saved, want_dx0=False)
    yield "backward", dict(zip(names, back.grads))
    back = ops.gmlp_train_backward(dy, x0, params, fwd.saved, want_dx0=True)
    yield "backward dx0", dict(zip(names + ["dx0"], back.grads + (back.dx0,)))


def head(shape, dev):
    x2, p, dlogits, running = H.sweep_case(shape, SEED, device=dev)
    rm, rv = running[0].clone(), running[1].clone()
    fwd = ops.head_train_forward(x2, *[p[k] for k in H.PARAMS], running_mean=rm, running_var=rv)
    yield "forward", {"logits": fwd.logits, "prob": fwd.prob, "running_mean": rm, "running_var": rv}
    back = ops.head_train_backward(dlogits, x2, p["w2"], p["wd"], p["gamma"], fwd.saved, want_dx2=True)
    yield "backward dx2", dict(zip(H.GRADS, back))


def linrelu(shape, dev):
    x, w, b, g = L.sweep_case(shape[0], shape[1], SEED, device=dev)
    y = ops.linrelu_train_forward(x, w, b).y
    yield "forward", {"y": y}
    back = ops.linrelu_train_backward(g, y, x, w, want_dx=True)
    yield "backward dx", dict(zip(L.GRADS, back))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("library:", _lib.LIB_PATH, file=sys.stderr)           # (not part of the listing: two listings must compare equal)
    lines, total = [], hashlib.sha256()
    for unit, run in (("rcab", rcab), ("gmlp", gmlp), ("head", head), ("linrelu", linrelu)):
        for shape in SHAPES[unit]:
            for case, tensors in run(shape, dev):
                for name, t in tensors.items():
                    data = np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()
                    total.update(data)
                    lines.append(f"{hashlib.sha256(data).hexdigest()}  {unit} {shape} {case}: {name}")
                    print(lines[-1], flush=True)
    lines.append(f"{total.hexdigest()}  all {len(lines)} tensors")
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
