#!/usr/bin/env python3
"""Record tests/golden/detector_loss.npz from the REFERENCE's own detector_loss on the CPU.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_detector_loss_golden.py

balf/loss/loss_function.py imports its package relatively, so the function body and tensor_op.pixel_shuffle_inv are compiled
from the reference's source with ``ast`` and run unchanged, as make_golden.py does.  Nothing of it is committed: the fixture
holds numbers only.

The reference draws its tie-break noise inside the call.  Per case: torch.manual_seed(s), draw
``torch.zeros(B,65,Hc,Wc).uniform_(0, 0.1)`` and store it; torch.manual_seed(s) again and call the reference with
``logits.requires_grad_()``; store the loss and ``logits.grad``.  That the stored noise is the one the reference used is
ASSERTED: the labels are recomputed from it and the loss is composed again on those labels
(tests/detector_loss_common.py: compose_f32); it must come out bit-identical to the reference's.

Also stored: loss64 / per_image64 / grad64 / labels of the float64 restatement (tests/detector_loss_common.py: restate64),
d_loss = max over cases of |loss_ref - loss64| / max(|loss64|, 1), d_grad = max over cases of |grad_ref - grad64| * den_b * B,
and the GPU gates tol_loss = max(4 * d_loss, 2^-21), tol_grad = max(4 * d_grad, 2^-21): the factor 4 because the device's
exp / log are not the CPU's libm (a rounding or two more per cell), the floor of eight float32 ulps so that an accidentally
tiny d does not make the gate unmeetable.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F                # (the reference's function body names it)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_functions                                  # noqa: E402
from tests.detector_loss_common import (FIXTURE, FIXTURE_CASES, TOL_FLOOR, compose_f32, grad_error, loss_error, make_case,  # noqa: E402
                                        restate64, space_to_depth)

REF = "/root/reference/balf/"


def reference_loss():
    top = ref_functions(REF + "utils/tensor_op.py", ["pixel_shuffle_inv"], {"torch": torch})
    ns = {"torch": torch, "F": F, "tensor_op": types.SimpleNamespace(pixel_shuffle_inv=top["pixel_shuffle_inv"])}
    return ref_functions(REF + "loss/loss_function.py", ["detector_loss"], ns)["detector_loss"], top["pixel_shuffle_inv"]


def main():
    ref, shuffle_inv = reference_loss()
    fx = {"meta.names": np.asarray([c[0] for c in FIXTURE_CASES])}
    d_loss = d_grad = 0.0
    for name, shape, seed, scale, with_mask in FIXTURE_CASES:
        case = make_case(shape, seed, scale, with_mask)
        b, hc, wc = shape
        torch.manual_seed(seed)
        noise = torch.zeros(b, 65, hc, wc).uniform_(0, 0.1)
        torch.manual_seed(seed)
        logits = case["logits"].clone().requires_grad_()
        loss = ref(case["keypoint_map"], logits, case["valid_mask"], 8, "cpu")
        loss.backward()
        # the stored noise reproduces the labels the reference used: the loss composed on them is the reference's, bit for bit
        assert torch.equal(shuffle_inv(case["keypoint_map"], 8), space_to_depth(case["keypoint_map"]))
        again = compose_f32(case["logits"], case["keypoint_map"], case["valid_mask"], noise)
        assert torch.equal(again, loss.detach()), (name, float(again), float(loss))
        vm = torch.ones_like(case["keypoint_map"]) if case["valid_mask"] is None else case["valid_mask"]
        vm = space_to_depth(vm).prod(dim=1)
        r = restate64(case["logits"], case["keypoint_map"], case["valid_mask"], noise)
        multi = int((space_to_depth(case["keypoint_map"]).sum(dim=1) > 1).sum())
        masked = int((vm == 0).sum())
        dl, dg = loss_error(loss.detach().numpy(), r["loss"]), grad_error(logits.grad.numpy(), r["grad"], r["den"])
        d_loss, d_grad = max(d_loss, dl), max(d_grad, dg)
        print(f"{name:10s} {shape} loss {float(loss):.7f} loss64 {float(r['loss']):.9f} d_loss {dl:.2e} d_grad {dg:.2e} "
              f"cells with several key points {multi}, masked cells {masked}, labels != 64: {int((r['labels'] != 64).sum())}")
        assert np.isfinite(float(loss)) and np.isfinite(logits.grad.numpy()).all()
        if name == "small":
            assert multi > 0 and masked > b                              # ties among key points; masked cells beyond the last image
        fx[f"{name}.logits"], fx[f"{name}.noise"] = case["logits"].numpy(), noise.numpy()
        fx[f"{name}.keypoint_map"] = case["keypoint_map"].numpy().astype(np.uint8)           # zeros and ones
        if with_mask:
            fx[f"{name}.valid_mask"] = case["valid_mask"].numpy().astype(np.uint8)
        fx[f"{name}.loss"], fx[f"{name}.grad"] = loss.detach().numpy(), logits.grad.numpy()
        fx[f"{name}.loss64"], fx[f"{name}.per_image64"], fx[f"{name}.grad64"] = r["loss"], r["per_image"], r["grad"]
        fx[f"{name}.labels"], fx[f"{name}.den64"] = r["labels"].astype(np.int32), r["den"]
    # a naive exp overflows on the logits x 100 case
    big = torch.from_numpy(fx["big_logits.logits"])
    assert not torch.isfinite(torch.log(torch.exp(big).sum(dim=1))).all()
    fx["d_loss"], fx["d_grad"] = np.float64(d_loss), np.float64(d_grad)
    fx["tol_loss"], fx["tol_grad"] = np.float64(max(4 * d_loss, TOL_FLOOR)), np.float64(max(4 * d_grad, TOL_FLOOR))
    print(f"d_loss {d_loss:.3e} d_grad {d_grad:.3e} tol_loss {float(fx['tol_loss']):.3e} tol_grad {float(fx['tol_grad']):.3e}")
    np.savez_compressed(FIXTURE, **fx)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
