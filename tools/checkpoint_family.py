#!/usr/bin/env python3
"""The checkpoint family of tests/golden/cases.py through the HIP forward: measured per member and requested precision.

    python tools/checkpoint_family.py [--out profiles/checkpoint_family.json] [--only SUB[,SUB...]]

Per row: the max-abs error of the score map against the float64 oracle (``err``; per image: noise, photograph), the fp32
oracle's own distance from it (``e32``), the split-path tolerance derived from it (``tol = max(2e-5, 4 e32)``), the precision the
module ended on, and -- for split-f16 requests -- what the split-f16 kernels THEMSELVES did on these weights, whatever the module
decided: their error (``err_split``) and their status block (``status``: score / range / se words of balf_forward_status).
tests/test_checkpoint_family_gpu.py asserts on the same measurement (it imports ``Family`` from here)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balf_amd import _lib, arch                                        # noqa: E402
from balf_amd.model import get_model                                   # noqa: E402
from balf_amd.utils import synth                                       # noqa: E402
from oracle import oracle as O                                         # noqa: E402
from tests.golden import cases                                         # noqa: E402

SPLIT_GATE = 2e-5        # the split-path gate of tests/test_forward_gpu.py::test_f16_split_forward_vs_reference_golden
CONTRACT = 1e-4          # the project's bar: validate_fp16's default, bench index_match.prob_max_abs_err


class Family:
    """One module object per requested precision, ``load_state_dict`` per member (the packed-weight cache notices).  The
    environment must allow the fall-back (BALF_FP16_STRICT unset) and look at the status block before forward returns
    (BALF_FP16_GUARD=sync): ``main`` sets both, the tests monkeypatch them."""

    def __init__(self, device="cuda:0"):
        self.dev = torch.device(device)
        self.sd0 = synth.synthetic_state_dict(cases.WEIGHT_SEED)
        self.x = cases.family_input(os.path.join(ROOT, "tests", "golden"))
        self.xg = self.x.to(self.dev)
        self.models = {}
        self._ref = {}

    def model(self, precision):
        if precision not in self.models:
            m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
            m.load_state_dict(self.sd0)
            m.precision = precision
            self.models[precision] = m.eval().to(self.dev)
        return self.models[precision]

    def reference(self, member):
        """-> (prob64 [2,H,W] float64, e32): the float64 oracle and the fp32 oracle's max-abs distance from it.  Exact members
        share the base member's: the fp32 oracle is bit-identical on this very input (tests/test_checkpoint_family.py)."""
        key = "base" if member[1] == "exact" else member[0]
        if key not in self._ref:
            sd = self.sd0 if key == "base" else cases.family_state(self.sd0, member)
            with torch.no_grad():
                p64 = O.detector_forward(O.cast_state(sd, torch.float64), self.x.double())["prob"].numpy()
                p32 = O.detector_forward(sd, self.x)["prob"].numpy()
            self._ref[key] = (p64, float(np.abs(p32 - p64).max()))
        return self._ref[key]

    def split_kernels(self, m):
        """The split-f16 kernels on the module's current weights through balf_forward_status with a status block of our own:
        -> (prob, status words).  Independent of what the module's probes and guard concluded."""
        l = _lib.lib()
        b, _, h, w = self.xg.shape
        blob = m.packed_weights(self.dev, "fp16")
        ws = torch.empty(l.balf_forward_workspace_bytes(b, h, w), dtype=torch.uint8, device=self.dev)
        prob = torch.empty((b, h, w), device=self.dev)
        status = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=self.dev)
        _lib.check(l.balf_forward_status(blob.data_ptr(), _lib.PREC_FP16, self.xg.data_ptr(), b, h, w, None, prob.data_ptr(),
                                         ws.data_ptr(), ws.numel(), status.data_ptr(), _lib.current_stream_ptr(self.dev)),
                   "balf_forward_status")
        torch.cuda.synchronize(self.dev)
        return prob.cpu().numpy(), status.cpu().tolist()

    def run(self, member, precision):
        """Load the member into the module of ``precision``, run the family input -> (row, prob as the caller got it)."""
        p64, e32 = self.reference(member)
        m = self.model(precision)
        m.load_state_dict(cases.family_state(self.sd0, member))
        with warnings.catch_warnings(record=True) as caught, torch.inference_mode():
            warnings.simplefilter("always")
            prob = m(self.xg, want_logits=False)["prob"].cpu().numpy()
        per_image = [float(v) for v in np.abs(prob - p64).max(axis=(1, 2))]
        row = {"member": member[0], "kind": member[1], "precision": precision, "effective": m.effective_precision,
               "err": max(per_image), "err_noise": per_image[0], "err_photo": per_image[1], "e32": e32,
               "tol": max(SPLIT_GATE, 4.0 * e32), "finite": bool(np.isfinite(prob).all()),
               "warned": sorted({str(c.message)[:60] for c in caught if issubclass(c.category, RuntimeWarning)})}
        if precision == "fp16":
            p16, words = self.split_kernels(m)
            row["status"] = words
            row["split_finite"] = bool(np.isfinite(p16).all())
            row["err_split"] = float(np.abs(p16 - p64).max()) if row["split_finite"] else None
        return row, prob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_family.json"))
    ap.add_argument("--only", default="", help="members whose id contains one of these (comma-separated)")
    a = ap.parse_args()
    os.environ.pop("BALF_FP16_STRICT", None)
    os.environ["BALF_FP16_GUARD"] = "sync"
    fam = Family()
    rows = []
    t0 = time.perf_counter()
    for member in cases.family_exact_members() + cases.family_dist_members():
        if not any(sub in member[0] for sub in a.only.split(",")):
            continue
        for precision in ("fp16", "fp32"):
            rows.append(fam.run(member, precision)[0])
    wall = time.perf_counter() - t0
    f16 = [r for r in rows if r["precision"] == "fp16"]
    kept = [r for r in f16 if r["effective"] == "fp16"]
    summary = {
        "members": len(f16), "wall_s": round(wall, 1), "input": list(cases.FAMILY_INPUT),
        "contract_1e-4_violations": [f"{r['member']}/{r['precision']}" for r in rows if not r["err"] <= CONTRACT],
        "kept_on_split_path": len(kept), "fell_back_to_fp32": sorted(r["member"] for r in f16 if r["effective"] != "fp16"),
        "kept_beyond_tol": sorted(r["member"] for r in kept if not r["err"] <= r["tol"]),
    }
    worst = sorted((r for r in f16 if r["err_split"] is not None), key=lambda r: -r["err_split"])[:8]
    # the file: one line per (pair, direction, k) with the four stages side by side, one line per other member.  err16: what the
    # fp16 request returned (worse of noise / photograph); split: the split kernels themselves; err32: the fp32 request
    g = lambda v: None if v is None else float(f"{v:.3e}")
    r32 = {r["member"]: r for r in rows if r["precision"] == "fp32"}
    groups = {}
    for r in f16:
        part = r["member"].split(".")
        stages = r["kind"] == "exact" and len(part) == 3
        groups.setdefault(f"{part[0]}.{part[2]}" if stages else r["member"], []).append(r)
    lines = [json.dumps({"member": name, "stages": [r["member"].split(".")[1] for r in rs] if len(rs) > 1 else None,
                         "e32": g(rs[0]["e32"]), "tol": g(rs[0]["tol"]), "effective": [r["effective"] for r in rs],
                         "err16": [g(r["err"]) for r in rs], "split": [g(r["err_split"]) for r in rs],
                         "status": [r["status"] for r in rs if any(r["status"])],
                         "err32": [g(r32[r["member"]]["err"]) for r in rs]}) for name, rs in groups.items()]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write('{"summary": ' + json.dumps(summary) + ',\n "rows": [\n  ' + ",\n  ".join(lines) + "\n]}\n")
    print(json.dumps({k: v for k, v in summary.items() if not k.startswith("worst")}))
    for r in worst:
        print("split kernels:", r["member"], f"err_split {r['err_split']:.2e} module err {r['err']:.2e} -> {r['effective']}", r["status"])


if __name__ == "__main__":
    main()
