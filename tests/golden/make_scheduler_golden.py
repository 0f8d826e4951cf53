#!/usr/bin/env python3
"""Record tests/golden/schedulers.json: the lr sequences of the REFERENCE's WarmRestart and LinearDecay.

Run in the build container only (the reference is mounted read-only at /root/reference and never travels to the GPU box):

    python tests/golden/make_scheduler_golden.py

balf/utils/train_utils.py imports cv2, tqdm and torchvision (absent offline), so the two class definitions are compiled from the
reference's source with ``ast`` and run unchanged, as make_val_golden.py does with functions.  The cases and the loop that reads the
sequence are tests/optim_common.py's (SCHEDULER_CASES, lr_sequence); tests/test_optim_host.py runs the same loop on
balf_amd.utils.train_utils' classes and asserts equality as floats.  The fixture holds numbers only."""
import ast
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.optim_common import BASE_LRS, EPOCHS, SCHEDULER_CASES, lr_sequence       # noqa: E402

REF = "/root/reference/balf/utils/train_utils.py"
NAMES = ("WarmRestart", "LinearDecay")


def ref_classes():
    tree = ast.parse(open(REF).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES)
    ns = {"optim": torch.optim, "math": math}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    return {k: ns[k] for k in NAMES}


def main():
    classes = ref_classes()
    fx = {"meta": {"epochs": EPOCHS, "base_lrs": list(BASE_LRS), "torch": torch.__version__,
                   "cases": {k: {"class": c, "kwargs": kw} for k, (c, kw) in SCHEDULER_CASES.items()}},
          "lr": {k: lr_sequence(classes, k) for k in SCHEDULER_CASES}}
    # what the fixture must show
    lr = {k: [row[0] for row in v] for k, v in fx["lr"].items()}
    assert lr["warm_default"][0] == lr["warm_default"][30] == lr["warm_default"][60] == BASE_LRS[0]       # two restarts
    assert lr["warm_default"][29] < 1e-5 and lr["warm_default"][59] < 1e-5
    assert lr["warm_mult"][20] == lr["warm_mult"][60] == BASE_LRS[0] and lr["warm_mult"][40] < BASE_LRS[0]  # the period doubled
    assert lr["linear_start_min"][10] == BASE_LRS[0] > lr["linear_start_min"][11]                          # flat, then falling
    assert lr["linear_resumed"][0] < BASE_LRS[0] and lr["linear_resumed_early"][0] == BASE_LRS[0]
    out = os.path.join(HERE, "schedulers.json")
    with open(out, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
