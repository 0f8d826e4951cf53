"""check_val_repeatability without a GPU: the fixture tests/golden/val_repeat.npz (recorded from the reference's own functions
by tests/golden/make_val_golden.py) is reproduced by a CPU composition of the oracle's pieces, the new entry points exist in
header, library and ctypes table, and the argument checks of the Python layer raise before anything touches a device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import val_repeat_common as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return V.fixture()


def test_fixture_is_small_and_complete(g):
    assert os.path.getsize(V.FIXTURE) <= 1 << 20
    names = [str(n) for n in g["meta.names"]]
    assert names[-1] == "last" and len(names) >= 5
    assert max(g["meta.batch_sizes"]) > 1
    assert g["shapes.prob_src"].shape != g["shapes.prob_dst"].shape
    k = int(g["meta.num_points"])
    for leg in V.LEGS:
        assert 0 < len(g[f"thin.{leg}.src"]) < k and 0 < len(g[f"thin.{leg}.dst"]) < k       # fewer than K positive values
        assert np.array_equal(g[f"zero.{leg}.src"][:, 0], np.arange(k)) and not g[f"zero.{leg}.src"][:, 3].any()   # raster fallback
    assert not g["black.image_src"].any() and not g["black.image_dst"].any()
    assert float(g["mild.greedy.rep_single_scale"]) > 50.0


def test_oracle_composition_reproduces_the_reference(g):
    """Counts equal, rows' positions and scores equal, floats within 1e-12 (the bar of test_repeat_batch_gpu.py)."""
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    for n in V.map_names(g):
        for leg in V.LEGS:
            src, dst, warped, r = V.oracle_pair(g[f"{n}.prob_src"], g[f"{n}.prob_dst"], g[f"{n}.h_dst_2_src"], nms, k, leg)
            assert np.array_equal(src, g[f"{n}.{leg}.src"]), (n, leg)
            assert np.array_equal(dst, g[f"{n}.{leg}.dst"]), (n, leg)
            assert warped.shape == g[f"{n}.{leg}.dst_to_src"].shape
            assert np.abs(warped - g[f"{n}.{leg}.dst_to_src"]).max() < 1e-12, (n, leg)
            for key in V.COUNT_KEYS + ("possible_matches",):
                assert int(r[key]) == int(g[f"{n}.{leg}.{key}"]), (n, leg, key)
            for key in V.REP_KEYS[:4]:
                assert abs(float(r[key]) - float(g[f"{n}.{leg}.{key}"])) < 1e-12, (n, leg, key)


def test_ten_means_from_the_per_pair_records(g):
    """The two quirks, stated on the recorded numbers: the first five are means over element 0 of every batch, the `_nms` five
    are the last pair's window-leg values and differ clearly from the window-leg mean."""
    names = [str(n) for n in g["meta.names"]]
    ten = g["loader.ten"]
    for i, key in enumerate(V.REP_KEYS):
        assert abs(ten[i] - np.mean([float(g[f"{n}.greedy.{key}"]) for n in names])) < 1e-12, key
        assert ten[5 + i] == float(g[f"last.window.{key}"]), key
    w_mean = np.mean([float(g[f"{n}.window.rep_single_scale"]) for n in names])
    assert abs(ten[5] - w_mean) > 1.0


def test_symbols_in_header_and_ctypes_table():
    from balf_amd import _lib
    header = open(os.path.join(ROOT, "include", "balf_hip.h")).read()
    for name in ("balf_val_points", "balf_val_points_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert "#define BALF_ABI_VERSION 1" in header
    assert (_lib.VAL_LEG_GREEDY, _lib.VAL_LEG_WINDOW) == (0, 1)
    assert "#define BALF_VAL_LEG_GREEDY 0" in header and "#define BALF_VAL_LEG_WINDOW 1" in header
    if os.path.isfile(_lib.LIB_PATH):
        l = _lib.lib()
        # host-side validation only: no device is touched by the size query
        assert l.balf_val_points_workspace_bytes(4, 128, 128, 128, 192, _lib.VAL_LEG_WINDOW, 15, 25) > 4 * 128 * 128 * 8
        assert l.balf_val_points_workspace_bytes(4, 128, 128, 128, 192, _lib.VAL_LEG_GREEDY, 15, 25) > 0
        assert l.balf_val_points_workspace_bytes(4, 128, 128, 128, 192, 2, 15, 25) == 0                    # no such leg
        assert l.balf_val_points_workspace_bytes(4, 4, 4, 128, 192, _lib.VAL_LEG_WINDOW, 15, 25) == 0      # K > h * w
        assert l.balf_val_points_workspace_bytes(4, 128, 128, 128, 128, _lib.VAL_LEG_GREEDY, 17, 25) == 0  # dist_thresh > 16
        assert l.balf_val_points_workspace_bytes(1, 4096, 8192, 64, 64, _lib.VAL_LEG_GREEDY, 1, 25) == 0   # keep bound > MAX_TOPK
        assert l.balf_val_points_workspace_bytes(0, 128, 128, 128, 128, _lib.VAL_LEG_WINDOW, 15, 25) == 0


def test_tb_log_raises():
    from balf_amd.utils import train_utils
    with pytest.raises(NotImplementedError):
        train_utils.check_val_repeatability([], None, "cpu", object(), 0)


def test_signature_matches_the_reference():
    import inspect
    from balf_amd.utils import train_utils
    p = list(inspect.signature(train_utils.check_val_repeatability).parameters.items())
    assert [n for n, _ in p[:8]] == ["dataloader", "model", "device", "tb_log", "cur_epoch", "cell_size", "nms_size", "num_points"]
    assert [v.default for _, v in p[5:8]] == [8, 15, 25]
    assert {"batch_size", "chunk_pairs"} <= {n for n, _ in p}
    # compute_repeatability_with_maximum_filter keeps its signature
    q = list(inspect.signature(train_utils.compute_repeatability_with_maximum_filter).parameters)
    assert q == ["src_scores_np", "dst_scores_np", "homography", "mask_src", "mask_dst", "nms_size", "num_points"]


def test_argument_checks():
    from balf_amd import ops
    from balf_amd._lib import BalfHipError
    from balf_amd.benchmark_test import evaluate
    from balf_amd.utils import train_utils
    prob = torch.zeros((2, 64, 64))
    h = torch.eye(3, dtype=torch.float64).expand(2, 3, 3).contiguous()
    with pytest.raises(ValueError):
        ops.val_points(prob, prob, h, 15, 25, "box")                    # no such leg
    with pytest.raises(BalfHipError):
        ops.val_points(prob, prob, h, 15, 25, "window")                 # host tensors: there is no CPU path
    with pytest.raises(BalfHipError):
        evaluate.evaluate_val_pairs(prob, prob, h, 15, 25, leg="greedy")
    with pytest.raises(ValueError):
        train_utils.check_val_repeatability([], None, "cpu", None, 0)   # an empty loader
