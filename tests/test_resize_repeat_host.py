"""The resize protocol without a GPU: the fixture tests/golden/resize_repeat.npz (recorded from the reference's own functions by
tests/golden/make_resize_golden.py) is reproduced by the NumPy restatement the GPU tests compare against,
adapt_homography_to_preprocessing is bit-identical to the recorded matrices, the new entry points exist in header, library and
ctypes table, and the argument checks return before anything touches a device."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import resize_repeat_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("balf_resize_repeatability_batch", "balf_resize_repeatability_batch_workspace_bytes", "balf_resize_crop_u8")


@pytest.fixture(scope="module")
def g():
    return R.fixture()


def test_fixture_is_small_and_complete(g):
    assert os.path.getsize(R.FIXTURE) <= 400 * 1024
    names = R.case_names(g)
    assert len(names) >= 12
    ks = {int(g[f"{n}.k"]) for n in names}
    ts = {float(g[f"{n}.thresh"]) for n in names}
    assert ks == {300, 1000} and ts == {1.0, 3.0, 5.0}
    assert tuple(g["unequal_shapes.shape_src"]) != tuple(g["unequal_shapes.shape_dst"])
    assert int(g["both_above_k.common_src_num"]) == 1000 == int(g["both_above_k.common_dst_num"])
    assert 0 < int(g["shift.common_src_num"]) < 300
    for n in ("empty_src", "empty_dst", "both_empty", "none_within"):
        assert float(g[f"{n}.repeatability"]) == 0.0 and float(g[f"{n}.localization_err"]) == -1.0
    src = g["rows.int.src"]
    assert np.array_equal(src[:, :2], np.floor(src[:, :2])) and np.array_equal(src[:, 2], src[:, 2].astype(np.float32))


def test_restatement_reproduces_the_reference(g):
    """Counts equal, repeatability bit-equal, localization_err within 1e-9 (the bound of the GPU test, derived there)."""
    for n in R.case_names(g):
        src, dst, h, ss, sd, k, thr = R.case_inputs(g, n)
        keep = src.copy()
        r, _, _ = R.resize_repeatability_np(src, dst, h, ss, sd, k, thr)
        assert np.array_equal(src, keep)
        for key in R.KEYS[2:]:
            assert int(r[key]) == int(g[f"{n}.{key}"]), (n, key)
        assert np.float64(r["repeatability"]) == np.float64(g[f"{n}.repeatability"]), n
        assert abs(float(r["localization_err"]) - float(g[f"{n}.localization_err"])) < 1e-9, n


def test_tie_rule_of_the_restatement():
    """Equal prob at the cut: the lower row index stays."""
    rows = np.array([[1.0, 1.0, 0.5], [2.0, 2.0, 0.7], [3.0, 3.0, 0.5], [4.0, 4.0, 0.5], [5.0, 5.0, 0.2]])
    assert np.array_equal(R.select_k_best(rows, 3)[:, 0], [1.0, 2.0, 3.0])
    assert np.array_equal(R.select_k_best(rows, 1)[:, 0], [2.0])
    assert np.array_equal(R.select_k_best(rows, 9)[:, 0], rows[:, 0])


def test_adapt_homography_is_bit_identical(g):
    from balf_amd.datasets import dataset_utils
    for i in range(len(g["adapt.out"])):
        z = {'homography': g["adapt.homography"][i], 'shape': g["adapt.shape"][i], 'warped_shape': g["adapt.warped_shape"][i]}
        keep = {k: v.copy() for k, v in z.items()}
        out = dataset_utils.adapt_homography_to_preprocessing(z, types.SimpleNamespace(resize_shape=list(g["adapt.target"][i])))
        assert out.dtype == g["adapt.out"].dtype and np.array_equal(out, g["adapt.out"][i]), i
        assert all(np.array_equal(z[k], keep[k]) for k in z)


def test_resize_restatement_geometry():
    """np.round is half to even; Python floor division for the offsets; imgaug's (top, right, bottom, left) order."""
    assert R.resize_geometry(480, 640, 240, 320) == (240, 320, 0, 0)
    assert R.resize_geometry(100, 500, 240, 320) == (240, 1200, 0, -440)
    assert R.resize_geometry(500, 100, 240, 320)[:2] == (1600, 320)
    assert R.resize_geometry(5, 8, 3, 4)[:2] == (3, 5)                     # scale = max(0.6, 0.5): 3.0, 4.8
    # an odd difference: floor division sends the extra pixel to the top crop (hp = -3) and to the RIGHT crop (left = -2)
    assert R.resize_geometry(240, 325, 240, 320) == (240, 325, 0, -2)
    assert R.resize_geometry(245, 320, 240, 320) == (245, 320, -3, 0)
    assert R.resize_geometry(3, 10, 3, 9) == (3, 10, 0, 0)
    assert R.resize_geometry(50, 25, 5, 2)[:2] == (5, 2)                   # 25 * 0.1 = 2.5 -> 2: half to even
    # 125 * 0.02 = 2.5 -> 2 (half to even), 175 * 0.02 = 3.5 -> 4
    assert int(np.round(2.5)) == 2 and int(np.round(3.5)) == 4
    img = np.arange(48, dtype=np.uint8).reshape(6, 8) * 5
    assert np.array_equal(R.ratio_preserving_resize_np(img, (6, 8)), img)  # same size: every weight is (2048, 0)
    out = R.ratio_preserving_resize_np(img, (3, 4))
    assert out.shape == (3, 4) and out.dtype == np.uint8
    rgb = np.stack([img, img // 2, 255 - img], axis=2)
    out3 = R.ratio_preserving_resize_np(rgb, (9, 7))
    assert out3.shape == (9, 7, 3) and np.array_equal(out3[..., 0], R.ratio_preserving_resize_np(img, (9, 7)))


def test_symbols_in_header_and_ctypes_table():
    from balf_amd import _lib
    header = open(os.path.join(ROOT, "include", "balf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["balf_resize_repeatability_batch"][1]) == 21
    assert len(_lib.PROTOTYPES["balf_resize_crop_u8"][1]) == 10
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name


def test_argument_checks_return_before_touching_a_device():
    from balf_amd import _lib
    l = _lib.lib()
    q = l.balf_resize_repeatability_batch_workspace_bytes
    assert q(64, 1000, 1000, 1000) >= 64 * (2 * 1000 * 8 + 2 * 1000 * 24)
    assert q(1, 0, 0, 1000) > 0                                            # empty sides are legal
    assert q(0, 10, 10, 10) == 0 and q(65536, 10, 10, 10) == 0
    assert q(1, 65537, 10, 10) == 0 and q(1, 10, -1, 10) == 0
    assert q(1, 10, 10, 0) == 0 and q(1, 10, 10, _lib.MAX_TOPK + 1) == 0
    fake = C.c_void_p(4096)
    f = l.balf_resize_repeatability_batch
    big = 1 << 40

    def call(src=fake, ns_max=10, s_stride=3, d_stride=3, c_stride=1, order=0, p=2, k=100, thr=5.0, ws_bytes=big, h_inv=fake):
        return f(src, fake, ns_max, s_stride, fake, fake, 10, d_stride, c_stride, order, p, fake, h_inv, fake, k, thr, fake, fake,
                 fake, ws_bytes, None)

    assert call(src=None) == -1 and call(h_inv=None) == -1
    assert call(s_stride=2) == -1 and call(d_stride=2) == -1 and call(c_stride=0) == -1
    assert call(order=1, s_stride=3) == -1 and call(order=2) == -1          # (x, y, r, score) rows need 4 columns
    assert call(p=0) == -1 and call(k=0) == -1 and call(ns_max=65537) == -1
    assert call(thr=-1.0) == -1 and call(thr=float("nan")) == -1
    assert call(ws_bytes=q(2, 10, 10, 100) - 1) == -3
    r = l.balf_resize_crop_u8
    assert r(None, 10, fake, fake, 1, 1, 8, 8, fake, None) == -1
    assert r(fake, 10, fake, fake, 0, 1, 8, 8, fake, None) == -1
    assert r(fake, 10, fake, fake, 1, 2, 8, 8, fake, None) == -1            # 1 or 3 channels
    assert r(fake, 10, fake, fake, 1, 3, 0, 8, fake, None) == -1
    assert r(fake, 10, fake, fake, 1, 3, 8, 16385, fake, None) == -2


def test_python_layer_raises_on_the_host():
    from balf_amd import ops
    from balf_amd._lib import BalfHipError
    from balf_amd.benchmark_test import evaluate, repeatability_tools
    from balf_amd.datasets import dataset_utils
    rows = torch.zeros((2, 5, 3), dtype=torch.float64)
    n = torch.zeros(2, dtype=torch.int32)
    h = torch.eye(3, dtype=torch.float64).expand(2, 3, 3).contiguous()
    sh = torch.tensor([[8, 8, 8, 8]] * 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.resize_repeatability_batch(rows, n, rows, n, h, h, sh, order="yx")
    with pytest.raises(ValueError):
        ops.resize_repeatability_batch(rows, n, rows, n, h, h, sh, keep_k_points=0)
    with pytest.raises(ValueError):
        ops.resize_repeatability_batch(rows, n, rows, n, h, h, sh, distance_thresh=-1)
    with pytest.raises(BalfHipError):
        ops.resize_repeatability_batch(rows, n, rows, n, h, h, sh)          # host tensors: there is no CPU path
    with pytest.raises(BalfHipError):
        repeatability_tools.compute_resize_repeatability_batch(rows, n, rows, n, h.numpy(), sh.numpy())
    with pytest.raises(BalfHipError):
        evaluate.evaluate_resize_pairs(rows, n, rows, n, h.numpy(), sh.numpy(), order="rcp")
    with pytest.raises(ValueError):
        dataset_utils.ratio_preserving_resize_batch([], (8, 8))
    with pytest.raises(ValueError):
        dataset_utils.ratio_preserving_resize_batch([np.zeros((4, 4), np.float32)], (8, 8))
    with pytest.raises(ValueError):
        dataset_utils.ratio_preserving_resize_batch([np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8)], (8, 8))


def test_signatures_match_the_reference():
    from balf_amd.benchmark_test import evaluate, repeatability_tools
    from balf_amd.datasets import dataset_utils
    p = inspect.signature(repeatability_tools.compute_resize_repeatability).parameters
    assert list(p) == ["keypoints", "warped_keypoints", "h", "shape_src", "shape_dst", "keep_k_points", "distance_thresh"]
    assert (p["keep_k_points"].default, p["distance_thresh"].default) == (1000, 5)
    assert list(inspect.signature(dataset_utils.adapt_homography_to_preprocessing).parameters) == ["zip_data", "args"]
    assert list(inspect.signature(dataset_utils.ratio_preserving_resize).parameters) == ["img", "target_size"]
    q = inspect.signature(evaluate.evaluate_resize_hsequences).parameters
    assert list(q)[:3] == ["dataloader", "model", "device"]
    assert (q["resize_shape"].default, q["top_k_points"].default, q["pixel_threshold"].default) == ((240, 320), 1000, 5)
    assert (q["nms_size"].default, q["border_size"].default) == (15, 15)
    assert {"chunk_sequences", "batch_size"} <= set(q)


def test_result_record_helpers():
    from balf_amd.benchmark_test import test_utils
    r = test_utils.create_reisze_results()
    assert list(r) == list(R.KEYS) and all(v == [] for v in r.values())
    assert r["repeatability"] is not r["localization_err"]
    m = test_utils.create_resize_metrics_results(["v_a", "i_b"], 1000, 5)
    assert list(m) == list(R.KEYS) + ["sequences", "top_k", "pixel_threshold"]
    assert m["sequences"] == ["v_a", "i_b"] and m["top_k"] == 1000 and m["pixel_threshold"] == 5
