"""The batched evaluation's host-side contract (no GPU): the C entry points check their sizes before any launch, the Python
entry points refuse host tensors instead of falling back to a CPU path."""
import numpy as np
import pytest
import torch

from balf_amd import _lib
from balf_amd.benchmark_test import evaluate, repeatability_tools as R
from balf_amd.utils import train_utils


def test_workspace_query_checks_the_limits():
    l = _lib.lib()
    assert l.balf_repeatability_batch_workspace_bytes(64, 1000, 1000, 1 << 20) > 48 * (1 << 20)
    assert l.balf_repeatability_batch_workspace_bytes(64, 65537, 10, 100) == 0          # N <= 65536 (LDS bitmaps)
    assert l.balf_repeatability_batch_workspace_bytes(1, 65536, 65536, 100) == 0        # ns * nd < 2^31
    assert l.balf_repeatability_batch_workspace_bytes(0, 10, 10, 100) == 0
    assert l.balf_repeatability_batch_workspace_bytes(4, 10, 10, 0) == 0


def test_entry_points_reject_bad_sizes_before_launching():
    l = _lib.lib()
    buf = (np.zeros(1 << 16, dtype=np.uint8))
    p = buf.ctypes.data
    args = (0.4, 1e-6, 3.0, 30.0, 100, p, p, p, buf.nbytes, None)
    assert l.balf_repeatability_batch(p, p, 65537, 4, p, p, 10, 4, 1, 2, *args) == -1       # BALF_ERR_ARG
    assert l.balf_repeatability_batch(p, p, 65536, 4, p, p, 65536, 4, 1, 1, *args) == -2    # BALF_ERR_SHAPE
    assert l.balf_repeatability_batch(p, p, 10, 2, p, p, 10, 4, 1, 1, *args) == -1          # rows need (x, y, radius)
    assert l.balf_repeatability_batch(p, p, 10, 4, p, p, 10, 4, 1, 1, 0.4, 1e-6, 3.0, 30.0, 100, p, p, p, 16, None) == -3
    assert l.balf_common_points_batch(p, p, 10, p, p, 10, 0, p, p, p, p, p, p, None) == -1
    assert l.balf_common_points_batch(p, p, 70000, p, p, 10, 1, p, p, p, p, p, p, None) == -1


def test_python_entry_points_have_no_cpu_path():
    src = torch.zeros((2, 5, 4), dtype=torch.float64)
    n = torch.full((2,), 5, dtype=torch.int32)
    with pytest.raises(_lib.BalfHipError):
        R.compute_repeatability_batch(src, n, src, n)
    with pytest.raises(_lib.BalfHipError):
        evaluate.evaluate_pairs(src, n, src, n, torch.eye(3, dtype=torch.float64).repeat(2, 1, 1),
                                torch.tensor([[100, 100, 100, 100]] * 2, dtype=torch.int32))


def test_driver_refuses_image_logging():
    class Loader:
        sequences = []

    with pytest.raises(NotImplementedError):
        train_utils.check_val_hsequences_repeatability(Loader(), None, "cpu", object(), 0)
