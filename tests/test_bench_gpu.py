"""bench.py's plain run on the GPU: it times --steps steps and prints the line with every --full leg left out, and
--dump-outputs writes the last timed step's outputs -- the same values for the same arguments, run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("other_precision", "with_logits", "allgather_device_us", "gathered_slabs_identical", "index_match", "cpu_baseline",
             "other_configs", "batch1_latency", "power_state_under_load", "sustained", "host_fed")
NAMES = ("keypoint_index", "keypoint_score", "keypoint_count", "prob_sample")


def test_plain_run_and_its_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch-per-gpu", "2", "--height", "480", "--width", "640", "--topk", "500",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        res = json.loads(lines[0])
        assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "images/s" and res["higher_is_better"] is True
        assert res["value"] == pytest.approx(2 * 1e3 / res["ms_per_step"], rel=1e-6)
        assert all(res[leg] is None for leg in FULL_ONLY), {leg: res[leg] for leg in FULL_ONLY if res[leg] is not None}
        dumps.append({n: np.load(d / f"{n}.npy") for n in NAMES})
    a, b = dumps
    assert a["keypoint_index"].dtype == np.float64 and a["keypoint_index"].shape == (2, 500)
    assert a["prob_sample"].dtype == np.float32 and a["prob_sample"].size == 2 * 512 * 640     # the whole padded map
    assert np.array_equal(a["keypoint_count"], (a["keypoint_index"] >= 0).sum(1)) and a["keypoint_count"].min() > 0
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
