"""The matching-score leg's host-side contract (no GPU): the result records, the two exported calls and their argument
checks before any launch, and the NumPy restatement of the definitions (tests/matching_common.py) on a hand-written case."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import _lib
from balf_amd.benchmark_test import evaluate, metrics_results, test_utils
from tests import matching_common as MC

RECORD_KEYS = {'num_features', 'rep_single_scale', 'rep_multi_scale', 'num_points_single_scale', 'num_points_multi_scale',
               'error_overlap_single_scale', 'error_overlap_multi_scale', 'mma', 'mma_corr', 'num_matches',
               'num_mutual_corresp', 'avg_mma'}


def test_result_records_have_the_reference_fields():
    r = metrics_results.create_results()
    assert set(r) == RECORD_KEYS and all(v == [] for v in r.values())
    assert len({id(v) for v in r.values()}) == len(r)            # one list each, not one list shared
    m = metrics_results.create_metrics_results(["a", "b"], 1000, 0.6, 5)
    assert set(m) == RECORD_KEYS | {'sequences', 'top_k', 'overlap', 'pixel_threshold'}
    assert (m['sequences'], m['top_k'], m['overlap'], m['pixel_threshold']) == (["a", "b"], 1000, 0.6, 5)
    # the reference's import path serves the same two constructors
    from balf_amd.benchmark_test.test_utils import create_metrics_results, create_results
    assert create_results is metrics_results.create_results and create_metrics_results is metrics_results.create_metrics_results
    # the resize protocol's records, in the module beside it, are as they were
    assert set(test_utils.create_resize_metrics_results([], 1000, 5)) == set(test_utils.RESIZE_RESULT_KEYS) | {
        'sequences', 'top_k', 'pixel_threshold'}


def test_library_exports_both_calls():
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "balf_common_points_index_batch") and hasattr(raw, "balf_match_accuracy_batch")
    l = _lib.lib()
    assert l.balf_abi_version() == 1                             # additive: the ABI version stays
    assert "balf_common_points_index_batch" in _lib.PROTOTYPES and "balf_match_accuracy_batch" in _lib.PROTOTYPES


def _th(*v):
    return (C.c_double * len(v))(*v)


def test_entry_points_reject_bad_arguments_before_launching():
    l = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    up = _th(*range(1, 11))
    acc = lambda ns=10, nd=10, cap=8, pairs=1, th=up, t=10, src=p, err=p: l.balf_match_accuracy_batch(       # noqa: E731
        src, ns, p, nd, p, p, p, cap, pairs, th, t, err, p, None)
    assert acc(t=0) == -1 and acc(t=17, th=_th(*range(1, 18))) == -1             # 1 <= T <= 16
    assert acc(th=_th(1, 2, 4, 3), t=4) == -1 and acc(th=_th(3, 2, 1), t=3) == -1   # not ascending
    assert acc(th=_th(1, 2, 2), t=3) == -1                                        # not strictly
    assert acc(th=_th(1, float("nan")), t=2) == -1 and acc(th=_th(-1, 2), t=2) == -1
    assert acc(pairs=0) == -1 and acc(pairs=65536) == -1                          # 1 <= P <= 65535
    assert acc(cap=0) == -1 and acc(cap=65537) == -1
    assert acc(ns=65537) == -1 and acc(ns=65536, nd=65536) == -2                  # as the neighbouring calls
    assert acc(src=None) == -1 and acc(err=None) == -1 and acc(th=None) == -1
    idx = lambda ns=10, nd=10, pairs=1, last=p: l.balf_common_points_index_batch(                            # noqa: E731
        p, p, ns, p, p, nd, pairs, p, p, p, p, p, p, p, last, None)
    assert idx(pairs=0) == -1 and idx(pairs=65536) == -1
    assert idx(ns=70000) == -1 and idx(ns=65536, nd=65536) == -2
    assert idx(last=None) == -1


def test_python_entry_points_check_their_arguments_and_have_no_cpu_path():
    src = torch.zeros((2, 5, 4), dtype=torch.float64)
    kept = torch.full((2, 2), 5, dtype=torch.int32)
    midx = torch.zeros((2, 5, 2), dtype=torch.int32)
    cnt = torch.full((2,), 5, dtype=torch.int32)
    ok = list(range(1, 11))
    bad = [
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx, cnt, []),                       # T = 0
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx, cnt, list(range(1, 18))),       # T = 17
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx, cnt, [3, 2, 1]),                # descending
        lambda: evaluate.match_accuracy_batch(src.float(), src, kept, midx, cnt, ok),               # dtype
        lambda: evaluate.match_accuracy_batch(src[0], src, kept, midx, cnt, ok),                    # rank
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx.long(), cnt, ok),                # dtype
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx[:, :, 0], cnt, ok),              # rank
        lambda: evaluate.match_accuracy_batch(src, src, kept[:, 0], midx, cnt, ok),                 # rank
        lambda: evaluate.match_accuracy_batch(src, src, kept, midx, cnt, ok),                       # host tensors: no CPU path
        lambda: evaluate.common_points_index_batch(src, cnt, src, cnt, torch.eye(3, dtype=torch.float64).repeat(2, 1, 1),
                                                   torch.tensor([[100, 100, 100, 100]] * 2, dtype=torch.int32)),
    ]
    for f in bad:
        with pytest.raises(_lib.BalfHipError):
            f()
    desc = torch.zeros((2, 5, 128))
    h = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    sh = torch.tensor([[100, 100, 100, 100]] * 2, dtype=torch.int32)
    with pytest.raises(_lib.BalfHipError, match="pixel_threshold"):
        evaluate.evaluate_matching_pairs(src, cnt, desc, src, cnt, desc, h, sh, pixel_threshold=11)
    with pytest.raises(_lib.BalfHipError, match="pixel_threshold"):
        evaluate.evaluate_matching_pairs(src, cnt, desc, src, cnt, desc, h, sh, thresholds=[1, 2, 3], pixel_threshold=5)
    with pytest.raises(_lib.BalfHipError, match="ascending"):
        evaluate.evaluate_matching_pairs(src, cnt, desc, src, cnt, desc, h, sh, thresholds=[5, 1], pixel_threshold=5)
    with pytest.raises(_lib.BalfHipError):
        evaluate.evaluate_matching_pairs(src, cnt, desc[:, :, :64], src, cnt, desc, h, sh)
    with pytest.raises(_lib.BalfHipError):
        evaluate.evaluate_matching_pairs(src, cnt, desc, src, cnt, desc, h, sh)                       # host tensors

    class Loader:
        sequences = []

    with pytest.raises(_lib.BalfHipError, match="pixel_threshold"):
        evaluate.evaluate_matching_hsequences(Loader(), None, None, "cpu", pixel_threshold=12)


def test_restatement_on_a_hand_written_case():
    """Four matches with errors 0, 3, 5 and 5.000001 pixels against the thresholds 1..10."""
    s = np.array([[10.0, 10.0, 1.0, 0.9], [20.0, 20.0, 1.0, 0.8], [30.0, 30.0, 1.0, 0.7], [40.0, 40.0, 1.0, 0.6]])
    d = np.array([[45.000001, 40.0, 1.0, 0.5], [33.0, 34.0, 1.0, 0.5], [20.0, 23.0, 1.0, 0.5], [10.0, 10.0, 1.0, 0.5]])
    matches = np.array([[0, 3], [1, 2], [2, 1], [3, 0]])
    e = MC.reprojection_errors(s, d, matches)
    assert e[0] == 0.0 and e[1] == 3.0 and e[2] == 5.0
    assert abs(e[3] - 5.000001) < 1e-12 and e[3] > 5.0
    correct = MC.correct_counts(e, range(1, 11))
    assert correct.tolist() == [1, 1, 2, 2, 3, 4, 4, 4, 4, 4]
    assert MC.correct_counts(e, [5]).tolist() == [3]
    # an index outside the lists: NaN, within no threshold
    e2 = MC.reprojection_errors(s, d, np.array([[0, 3], [4, 0], [0, -1]]))
    assert e2[0] == 0.0 and np.isnan(e2[1]) and np.isnan(e2[2])
    assert MC.correct_counts(e2, [1, 10]).tolist() == [1, 1]
    # the ratios: 3 of 4 within 5 px; the mean over the ten thresholds
    assert MC.ratio(3, 4) == 0.75 and MC.ratio(3, 0) == 0.0
    avg = 0.0
    for c in correct:
        avg += c / 4.0
    assert avg / 10.0 == (1 + 1 + 2 + 2 + 3 + 4 * 5) / 4.0 / 10.0
