"""NMS score maps (balf_nms_score_map) without a GPU: the NumPy oracle of tests/nms_map_common.py against the
fixture recorded from the reference, the host-side footprint table, and every refusal that comes before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd._lib import BalfHipError
from balf_amd.benchmark_test import repeatability_tools
from balf_amd.utils import train_utils
from tests import nms_map_common as M


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def test_fixture_inputs_are_what_the_recorder_saw(fx):
    scores = [fx[f"{c}.score"] for c in M.CASES]
    assert str(fx["inputs_sha256"]) == M.digest(*scores)
    for name in M.SYNTH_SHAPES:
        assert M.same_map(fx[f"{name}.score"], M.synthetic_scores(name))
    for s in scores:                                            # the reference is defined: every candidate score distinct
        cand = s[s >= np.float32(M.CONF)]
        assert len(np.unique(cand)) == len(cand) > 0 and (s < np.float32(M.CONF)).any()


def test_oracle_equals_the_reference_exactly(fx):
    cases = M.fixture_cases(fx)
    assert len(cases) == len(M.CASES) * (len(M.BOX_ARGS) + len(M.GREEDY_DISTS))
    for case, score, label, want, call in cases:
        if call[0] == "box":
            got, n = M.box_oracle(score, call[1], call[2], M.CONF, call[3])
        else:
            got, n = M.greedy_oracle(score, call[1], M.CONF)
        assert M.same_map(got, want), (case, label)
        assert n == np.count_nonzero(want), (case, label)


@pytest.mark.parametrize("size,iou", [(4, 0.1), (4, 0.5), (3, 0.1), (8.5, 0.1), (17, 0.3), (1, 0.1)])
def test_box_footprint_is_the_float32_iou_over_all_offsets(size, iou):
    radius, rows = ops.box_footprint(size, iou)
    assert radius == int(np.ceil(size)) - 1 and len(rows) == 2 * radius + 1
    reach = radius + 2                                           # nothing beyond the radius overlaps at all
    _, inside = M.box_footprint_direct(size, iou, reach=reach)
    for dr in range(-reach, reach + 1):
        for dc in range(-reach, reach + 1):
            in_table = abs(dr) <= radius and abs(dc) <= radius and bool((rows[dr + radius] >> (dc + radius)) & 1)
            assert in_table == bool(inside[dr + reach, dc + reach]), (size, iou, dr, dc)
    assert all(r >> (2 * radius + 1) == 0 for r in rows)
    if size == 1:
        assert radius == 0 and rows == (1,)                      # the centre alone


def test_default_footprint_is_no_rectangle():
    radius, rows = ops.box_footprint(4, 0.1)
    has = lambda dr, dc: bool((rows[dr + radius] >> (dc + radius)) & 1)      # noqa: E731
    assert radius == 3
    assert has(3, 0) and has(3, 1) and not has(3, 2)
    assert has(0, 3) and has(1, 3) and not has(2, 3) and has(-3, -1) and not has(-3, -2)


@pytest.mark.parametrize("size,iou", [(4.25, 0.1), (3.3, 0.1), (0, 0.1), (-4, 0.1), (17.5, 0.1), (18, 0.1), (4, 1.0), (4, -0.1),
                                      (4, float("nan")), (float("nan"), 0.1)])
def test_box_footprint_refuses(size, iou):
    with pytest.raises(ValueError):
        ops.box_footprint(size, iou)


FAKE = 4096            # a non-null address that is never dereferenced: every refusal below comes before any launch


def _call(lib, b=1, h=40, w=72, protocol=_lib.NMS_MAP_BOX, conf=0.015, dist=4, rows=(1,), radius=0, k=-1, prob=FAKE, out=FAKE,
          ws=FAKE, ws_bytes=1 << 40):
    table = (C.c_uint64 * max(len(rows), 1))(*rows) if rows is not None else None
    return lib.balf_nms_score_map(prob, b, h, w, protocol, conf, dist, table, radius, k, out, None, ws, ws_bytes, None)


def test_c_abi_refuses_before_any_launch():
    lib = _lib.lib()
    n = C.c_size_t(12345)
    for args in ((1, 40, 72, 2), (1, 40, 72, -1), (0, 40, 72, 0), (1, 0, 72, 0), (1, 40, -3, 1), (65536, 40, 72, 1)):
        assert lib.balf_nms_score_map_sizes(*args, C.byref(n)) == -1, args
        assert n.value == 12345                                  # untouched
    assert lib.balf_nms_score_map_sizes(1, 65536, 65536, 0, C.byref(n)) == -2 and n.value == 12345
    assert lib.balf_nms_score_map_sizes(1, 40, 72, 0, None) == -1
    for protocol in (_lib.NMS_MAP_GREEDY, _lib.NMS_MAP_BOX):
        assert lib.balf_nms_score_map_sizes(2, 40, 72, protocol, C.byref(n)) == 0 and n.value >= 2 * 40 * 72 * 8
    # the entry point: null pointers first, then each bad argument with pointers that would pass
    assert lib.balf_nms_score_map(None, 1, 40, 72, 1, 0.015, 4, None, 0, -1, None, None, None, 0, None) == -1
    assert _call(lib, protocol=2) == -1 and _call(lib, protocol=-1) == -1
    assert _call(lib, b=0) == -1 and _call(lib, h=0) == -1 and _call(lib, w=-1) == -1 and _call(lib, b=65536) == -1
    assert _call(lib, h=65536, w=65536) == -2
    for d in (0, 17, -1):
        assert _call(lib, protocol=_lib.NMS_MAP_GREEDY, dist=d) == -1, d
    assert _call(lib, radius=17, rows=(1,) * 35) == -1 and _call(lib, radius=-1) == -1
    assert _call(lib, rows=None) == -1                            # BOX without a table
    assert _call(lib, radius=1, rows=(0b010, 0b101, 0b010)) == -1      # without the centre
    assert _call(lib, radius=1, rows=(0b011, 0b111, 0b011)) == -1      # not symmetric
    assert _call(lib, radius=1, rows=(0b1010, 0b111, 0b010)) == -1     # a bit beyond the table
    for conf in (0.0, -0.015, float("nan")):
        assert _call(lib, conf=conf) == -1
    for kw in ({"prob": None}, {"out": None}, {"ws": None}):
        assert _call(lib, **kw) == -1, kw
    assert _call(lib, ws_bytes=n.value - 1, b=2) == -3            # one byte short of the queried size


def test_python_functions_raise_the_projects_errors():
    cpu = torch.zeros((1, 40, 72), dtype=torch.float32)
    with pytest.raises(BalfHipError, match="GPU"):
        ops.nms_score_map(cpu, "box", conf_thresh=0.015, size=4, iou=0.1)
    with pytest.raises(BalfHipError, match="GPU"):
        repeatability_tools.box_nms(cpu)
    with pytest.raises(BalfHipError, match="GPU"):
        repeatability_tools.box_nms_batch(cpu)
    with pytest.raises(BalfHipError, match="GPU"):
        repeatability_tools.nms_fast_score_map_batch(cpu, 4)
    with pytest.raises(BalfHipError, match="GPU"):
        train_utils.prob_to_score_maps_tensor_batch(cpu, 4)
    for bad in (torch.zeros((40, 72)), torch.zeros((1, 1, 40, 72)), torch.zeros((1, 40, 72), dtype=torch.float64)):
        with pytest.raises(BalfHipError, match=r"\[B,H,W\] float32"):
            ops.nms_score_map(bad, "greedy", conf_thresh=0.015, dist_thresh=4)
    for bad in (torch.zeros((2, 40, 72)), torch.zeros((40, 72)), np.zeros((1, 40, 72), np.float32)):
        with pytest.raises(BalfHipError, match=r"\[1,H,W\]"):
            repeatability_tools.box_nms(bad)
    with pytest.raises(ValueError, match="protocol"):
        ops.nms_score_map(cpu, "window", conf_thresh=0.015)
    for fn in (repeatability_tools.apply_nms_fast, repeatability_tools.get_nms_score_map_from_score_map):
        with pytest.raises(ValueError, match=r"\[H, W\]"):
            fn(np.zeros((1, 40, 72), np.float32), 4)
    if not torch.cuda.is_available():
        with pytest.raises(BalfHipError, match="no CPU path"):
            repeatability_tools.apply_nms_fast(np.zeros((40, 72), np.float32), 4)
        with pytest.raises(BalfHipError, match="no CPU path"):
            repeatability_tools.get_nms_score_map_from_score_map(np.zeros((40, 72), np.float32))
