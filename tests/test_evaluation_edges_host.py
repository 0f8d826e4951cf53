"""The references and generators of the evaluation-leg edge tests (tests/evaluation_common.py) checked without a GPU: the
references against the recorded goldens (repeatability.npz, resize_repeat.npz, val_repeat.npz) and against independent
statements, the generators against the properties the GPU tests rely on (boundary rows carry candidates, no overlap near the
threshold, both ping-pong parities, nearest neighbours in every LDS tile), and the size limits the C entry points check before
any launch."""
import os

import numpy as np
import pytest

from balf_amd import _lib
from balf_amd.benchmark_test import repeatability_tools as R
from oracle import oracle as O
from tests import evaluation_common as E
from tests import resize_repeat_common as RR
from tests import val_repeat_common as V
from tests.golden import cases

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the references against the goldens -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.REPEAT_CASES))
def test_overlaps_reproduce_the_repeatability_golden(name):
    """overlaps_np + the oracle's greedy assignment give the recorded counts and errors; the candidate counts bound them."""
    g = np.load(os.path.join(HERE, "golden", "repeatability.npz"))
    spec = cases.REPEAT_CASES[name]
    src, dst = cases.repeat_inputs(spec)
    kw = dict(spec["kw"])
    overlap_err = kw.pop("overlap_err", 0.4)
    kw.pop("dist_match_thresh", None)
    single, multi = E.overlaps_np(src, dst, **kw)
    _, totals = E.candidate_counts(src, dst, overlap_err=overlap_err, **kw)
    for which, (mat, scale) in enumerate(((single, "single_scale"), (multi, "multi_scale"))):
        found, err, _ = O._greedy_assign(mat, 1 - overlap_err)
        assert found == int(g[f"{name}.num_points_{scale}"])
        want = float(g[f"{name}.error_overlap_{scale}"])
        assert abs((0.0 if found == 0 else err / float(found + np.finfo(float).eps)) - want) < 1e-12
        assert totals[which] >= found and totals[which] == int((mat >= 1 - overlap_err).sum())


def test_resize_reference_reproduces_the_resize_golden():
    g = RR.fixture()
    for n in RR.case_names(g):
        src, dst, h, ss, sd, k, thr = RR.case_inputs(g, n)
        if ss != sd:
            continue                                                 # (resize_reference takes one shape; the others pin it)
        res, (arg1, min1), (arg2, min2), (n1, n2) = E.resize_reference(src, dst, k, thr, h, ss)
        for key in RR.KEYS[2:]:
            assert int(res[key]) == int(g[f"{n}.{key}"]), (n, key)
        assert np.float64(res["repeatability"]) == np.float64(g[f"{n}.repeatability"]), n
        assert abs(float(res["localization_err"]) - float(g[f"{n}.localization_err"])) < 1e-9, n
        assert (n1, n2) == (res["common_src_num"], res["common_dst_num"]) and len(arg1) == len(min1) == (n1 if n2 else 0)


@pytest.mark.parametrize("leg", V.LEGS)
def test_val_select_reproduces_the_validation_golden(leg):
    """The masked NMS maps from the oracle's pieces + val_select are the recorded rows, bit for bit."""
    g = V.fixture()
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    for n in V.map_names(g):
        ps, pd, h = g[f"{n}.prob_src"], g[f"{n}.prob_dst"], g[f"{n}.h_dst_2_src"]
        ms, md = O.create_common_region_masks(h, ps.shape, pd.shape, numpy_inverse=False)
        got_s = E.val_select(np.multiply(V.oracle_nms_map(ps, nms, leg), ms), k)
        got_d = E.val_select(np.multiply(V.oracle_nms_map(pd, nms, leg), md), k)
        assert np.array_equal(got_s.view(np.uint64), g[f"{n}.{leg}.src"].view(np.uint64)), (n, leg)
        assert np.array_equal(got_d.view(np.uint64), g[f"{n}.{leg}.dst"].view(np.uint64)), (n, leg)


def test_check_common_points_reference():
    """Equal to the package's host check_common_points where NumPy accepts every index; the 31 x 31 mask is the single pixel
    (15, 15), the 30 x 30 one is empty; unusable coordinates are dropped and nothing else."""
    rng = np.random.default_rng(5)
    ms, md = O.create_common_region_masks(cases.HOMOGRAPHY, (240, 320), (240, 320), numpy_inverse=False)
    pts = np.stack([rng.uniform(-0.49, 319.49, 2000), rng.uniform(-0.49, 239.49, 2000)], axis=1)       # rint - 1 in [-1, n - 1]
    for mask in (ms, md):
        assert np.array_equal(E.check_common_points_np(pts, mask), R.check_common_points(pts[:, ::-1], mask))
    ms, md = O.create_common_region_masks(np.eye(3), (31, 31), (31, 31), numpy_inverse=False)
    assert ms.sum() == 1 and ms[15, 15] == 1 and md.sum() == 1 and md[15, 15] == 1
    ms, _ = O.create_common_region_masks(np.eye(3), (30, 30), (30, 30), numpy_inverse=False)
    assert ms.sum() == 0
    by_name = {c["name"]: c for c in E.common_cases()}
    c = by_name["31x31"]
    ks, kd, i_s, i_d = E.common_points_ref(c["src"], c["dst"], c["h"], c["shapes"])
    assert [tuple(r[:2]) for r in ks] == [(16.0, 16.0), (16.4, 15.6), (16.5, 16.5)] and list(i_s) == [0, 2, 5]
    c = by_name["bad_coordinates"]
    ks, _, i_s, _ = E.common_points_ref(c["src"], c["dst"], c["h"], c["shapes"])
    usable = np.isfinite(c["src"][:, :2]).all(axis=1) & (np.abs(c["src"][:, :2]) < 1e9).all(axis=1) & (c["src"][:, :2] >= 0).all(axis=1)
    assert list(i_s) == list(np.flatnonzero(usable)) and 0 < len(i_s) < len(c["src"])
    for name in ("singular", "zero_shape", "negative_shape", "30x30"):
        c = by_name[name]
        assert all(len(a) == 0 for a in E.common_points_ref(c["src"], c["dst"], c["h"], c["shapes"])), name
    for name, sides in (("one_side_empty", (0, 80)), ("inside_255_513", (255, 513)), ("inside_513_255", (513, 255))):
        c = by_name[name]
        ks, kd, _, _ = E.common_points_ref(c["src"], c["dst"], c["h"], c["shapes"])
        assert (len(ks), len(kd)) == sides, name
    c = by_name["perspective"]
    ks, kd, _, _ = E.common_points_ref(c["src"], c["dst"], c["h"], c["shapes"])
    assert 0 < len(ks) < len(c["src"]) and 0 < len(kd) < len(c["dst"])
    a, b, cc, d, e, f, gg, hh, i = E.SINGULAR_H.ravel()
    assert a * (e * i - f * hh) + b * -(d * i - f * gg) + cc * (d * hh - e * gg) == 0.0


@pytest.mark.parametrize("cap", E.MATCH_CAPS)
def test_match_accuracy_reference(cap):
    """Every finite error of the generated matches is one of 0, sqrt 2, 5, 10, 13 exactly; a threshold at such a value counts
    it, the float just below does not; clamped counts and bad indices give NaN."""
    c = E.match_case(cap)
    err, correct = E.match_accuracy_np(c["src"], c["dst"], c["kept"], c["match_idx"], c["match_count"], E.THRESHOLDS_16)
    finite = err[np.isfinite(err)]
    assert set(np.unique(finite)) <= {0.0, np.sqrt(2.0), 5.0, 10.0, 13.0}
    assert np.isnan(err[2]).all() and not correct[2].any()                         # negative count
    assert np.isfinite(err[1]).all() and np.isfinite(err[3]).all()                 # count above cap / kept above n_max: clamped
    assert np.isnan(err[4, ::7]).all() and (cap < 8 or np.isfinite(err[4, 1:7]).all())
    assert cap < 255 or (np.isnan(err[5]).any() and np.isfinite(err[5]).any())
    th = list(E.THRESHOLDS_16)
    for v in (5.0, 10.0, 13.0):
        at, lo = th.index(v), th.index(E.below(v))
        assert lo == at - 1 and np.array_equal(correct[:, at] - correct[:, lo], (err == v).sum(axis=1))
    assert np.array_equal(correct[:, -1], np.isfinite(err).sum(axis=1))
    if cap >= 255:
        assert all((finite == v).any() for v in (5.0, 10.0, 13.0))
    one, c1 = E.match_accuracy_np(c["src"], c["dst"], c["kept"], c["match_idx"], c["match_count"], E.THRESHOLDS_1[0])
    _, c0 = E.match_accuracy_np(c["src"], c["dst"], c["kept"], c["match_idx"], c["match_count"], E.THRESHOLDS_1[1])
    assert np.array_equal(one, err, equal_nan=True) and np.array_equal(c1[:, 0] - c0[:, 0], (err == 5.0).sum(axis=1))


# ---- the generators ---------------------------------------------------------------------------------------------------------
def test_row_scan_boundary_rows_carry_candidates():
    pairs = E.row_scan_pairs()
    assert tuple(len(s) for s, _ in pairs) == E.ROW_SCAN_NS and tuple(len(d) for _, d in pairs) == E.ROW_SCAN_ND
    seen = set()
    for src, dst in pairs[:4]:
        rows, totals = E.candidate_counts(src, dst)
        assert E.threshold_margin(src, dst) > E.THR_MARGIN
        assert totals[0] > totals[1] > 0                             # the radius-2 rows are single-scale candidates only
        for r in E.BOUNDARY_ROWS:
            if r < len(src):
                assert rows[r].min() >= 1, r
                seen.add(r)
        for lo in (1023, 2047):                                      # different counts on the two sides of a chunk edge
            if lo + 1 < len(src):
                assert rows[lo, 0] != rows[lo + 1, 0] and rows[lo, 1] != rows[lo + 1, 1]
        # the running sum is not flat before the edge either
        assert (rows[:1000].sum(axis=0) > 20).all()
    assert seen == set(E.BOUNDARY_ROWS)
    src, dst = pairs[4]
    s, _ = E.overlaps_np(src, dst)
    assert set(np.flatnonzero((s >= 0.6).any(axis=0))) == {0, 63, 64, 1023, 1024, 2048}
    assert E.threshold_margin(src, dst) > E.THR_MARGIN


def test_pair_scan_pairs_around_the_chunk_edges_are_not_empty():
    pairs = E.pair_scan_pairs()
    assert len(pairs) == E.PAIR_SCAN_P
    totals = np.array([E.candidate_counts(s, d)[1] for s, d in pairs])
    ns, nd = np.array([len(s) for s, _ in pairs]), np.array([len(d) for _, d in pairs])
    assert ns.max() == nd.max() == E.PAIR_SCAN_N and (ns == 0).sum() > 100 and (nd == 0).sum() > 100
    for p in E.PAIR_SCAN_NONEMPTY:
        assert totals[p].min() >= 1, p
    assert (totals[:1024].sum(axis=0) > 1000).all()                 # the carry into the second chunk is not small
    assert min(E.threshold_margin(s, d) for s, d in pairs) > E.THR_MARGIN


def test_overflow_pairs_have_candidates_in_both_scales():
    for src, dst in E.overflow_pairs():
        _, totals = E.candidate_counts(src, dst)
        assert totals[0] > totals[1] > 0 and E.threshold_margin(src, dst) > E.THR_MARGIN


def test_sort_inputs_feed_both_ping_pong_outcomes():
    """All-equal keys: no digit differs (every pass skipped).  Few-valued keys: the number of differing digits, i.e. of passes
    that run, is odd for some lists and even for others."""
    for a, b in E.EQUAL_KEY_SHAPES:
        for keys in E.candidate_keys(*E.equal_key_pair(a, b)):
            assert len(keys) == a * b and E.differing_nibbles(keys) == 0
    assert [a * b for a, b in E.EQUAL_KEY_SHAPES] == [1, 63, 64, 65, 1023, 1024, 1025, 1089, 2070]
    parities = set()
    for case in E.FEW_KEY_CASES:
        src, dst = E.few_key_pair(case)
        assert E.threshold_margin(src, dst) > E.THR_MARGIN
        for keys in E.candidate_keys(src, dst):
            assert 2 <= len(np.unique(keys)) <= 4 and len(keys) > 60
            parities.add(E.differing_nibbles(keys) % 2)
    assert parities == {0, 1}


def test_word_edge_and_limit_inputs():
    for ns in E.WORD_EDGES:
        for nd in E.WORD_EDGES:
            src, dst = E.word_edge_pair(ns, nd)
            assert (len(src), len(dst)) == (ns, nd) and E.threshold_margin(src, dst) > E.THR_MARGIN
            _, totals = E.candidate_counts(src, dst)
            r = E.oracle_repeatability(src, dst)
            # rows compete: more candidates than assignments, and most rows of the shorter side find a partner
            assert totals[0] > r["num_points_single_scale"] >= min(ns, nd) - 8
            for key in ("correspondences", "correspondences_m"):     # the last index of both sides is set, then consulted
                got = {tuple(c) for c in r[key]}
                assert {(nd - 1, ns - 1), (nd - 2, ns - 2)} <= got and (nd - 1, ns - 2) not in got
    for side in (0, 1):
        src, dst = E.limit_pair(side)
        assert max(len(src), len(dst)) == E.MAX_ROWS and min(len(src), len(dst)) == 2
        assert E.threshold_margin(src, dst) > E.THR_MARGIN
        s, _ = E.overlaps_np(src, dst)
        hit = np.flatnonzero((s >= 0.6).any(axis=1 - side))
        assert {0, 1023, 1024, 32768, 65504, 65535} <= set(hit) and len(hit) == 10


@pytest.mark.parametrize("case", E.RESIZE_CASES)
def test_resize_nearest_neighbours_sit_in_every_tile(case):
    """Among the minima within the threshold, in the direction whose columns are the long side's kept rows (K of them) and in
    the other one, the nearest column lies in every LDS tile the column list spans and at column n_col - 1."""
    k = case[0]
    for long_is_src in (True, False):
        src, dst = E.resize_case(*case, long_is_src)
        res, (arg1, min1), (arg2, min2), (n1, n2) = E.resize_case_reference(*case, long_is_src)
        assert (n1, n2) == ((k, case[2]) if long_is_src else (case[2], k))
        assert (len(src) > k > len(dst)) if long_is_src else (len(dst) > k > len(src))
        for arg, mins, n_col in ((arg1, min1, n2), (arg2, min2, n1)):
            near = arg[mins <= E.RESIZE_THRESH]
            tiles = set(near // E.MIN_TILE)
            assert tiles == set(range((n_col + E.MIN_TILE - 1) // E.MIN_TILE)), (case, long_is_src, n_col)
            assert n_col - 1 in near
        assert res["rep_src_num"] > 100 and res["rep_dst_num"] > 100
        assert src[:, :2].max() < 4096 and dst[:, :2].max() < 4096   # the bound the localization_err tolerance assumes


def test_signed_zero_cut_separates_the_two_orders():
    src, dst, h, ss, sd, k, thr = E.signed_zero_case()
    want, _, _ = RR.resize_repeatability_np(src, dst, h, ss, sd, k, thr)
    assert (want["common_src_num"], want["common_dst_num"], want["rep_src_num"], want["rep_dst_num"]) == (20, 20, 20, 20)
    assert np.signbit(src[10:25, 2]).all() and not np.signbit(src[25:, 2]).any() and not src[10:, 2].any()
    # an order that ranks -0.0 below +0.0 keeps rows 25..34 instead of 10..19
    other = np.r_[0:10, 25:35]
    wrong, _, _ = RR.resize_repeatability_np(src[other], dst[other], h, ss, sd, k, thr)
    assert (wrong["rep_src_num"], wrong["rep_dst_num"]) == (10, 10)


def test_val_maps_reach_every_branch_of_the_selection():
    """Per map kind, from the masked NMS maps: dense has more than K positive values with distinct scores at the cut, levels
    has a tie at the cut (more values reach the threshold than K), sparse has fewer than K positive values, zero and the
    masked-out pair have none."""
    shapes = E.VAL_SHAPES[0]
    for leg, nms, big in (("window", 1, 6000), ("greedy", 1, 1025)):
        maps = {(b, p): E.val_masked_maps(b, shapes, leg, nms)[p] for b in (0, 1) for p in range(3)}
        kinds = {(b, p): E.VAL_BATCHES[b][p] for b in (0, 1) for p in range(3)}
        for key, (kind, h) in kinds.items():
            for m in maps[key]:
                pos = int((m > 0).sum())
                if kind == "zero" or h is E.VAL_GONE:
                    assert pos == 0
                elif kind == "sparse":
                    assert 0 < pos < 1023
                elif kind == "levels":
                    assert pos > big and int((m >= O.topk_threshold(m, 1024)).sum()) > 1024
                else:
                    assert pos > big and int((m >= O.topk_threshold(m, 1024)).sum()) == 1024
    # the greedy leg with nms_size 1 keeps at most one point per 2 x 2 cell: fewer than K = 6000 rows
    assert all(int((m > 0).sum()) <= 4096 for pair in E.val_masked_maps(0, shapes, "greedy", 1) for m in pair)


# ---- the limits the C entry points check before any launch ------------------------------------------------------------------
def test_size_limits_are_checked_on_the_host():
    l = _lib.lib()
    buf = np.zeros(1 << 12, dtype=np.uint8)
    p = buf.ctypes.data
    rep = (0.4, 1e-6, 3.0, 30.0, 100)
    assert l.balf_repeatability(p, E.MAX_ROWS + 1, p, 2, *rep, p, p, p, p, p, buf.nbytes, None) == -1
    assert l.balf_repeatability(p, 2, p, E.MAX_ROWS + 1, *rep, p, p, p, p, p, buf.nbytes, None) == -1
    assert l.balf_repeatability_workspace_bytes(E.MAX_ROWS, 2, 100) > 0
    assert l.balf_repeatability_batch(p, p, E.MAX_ROWS + 1, 4, p, p, 2, 4, 1, 1, *rep, p, p, p, buf.nbytes, None) == -1
    assert l.balf_repeatability_batch(p, p, 2, 4, p, p, E.MAX_ROWS + 1, 4, 1, 1, *rep, p, p, p, buf.nbytes, None) == -1
    assert l.balf_repeatability_batch_workspace_bytes(1, E.MAX_ROWS, 2, 100) > 0
    assert l.balf_common_points_index_batch(p, p, E.MAX_ROWS + 1, p, p, 2, 1, p, p, p, p, p, p, p, p, None) == -1

    def accuracy(cap, ths):
        arr = (_lib.C.c_double * len(ths))(*ths)
        return l.balf_match_accuracy_batch(p, 10, p, 10, p, p, p, cap, 1, arr, len(ths), p, p, None)

    assert accuracy(10, [float(t) for t in range(17)]) == -1                       # T = 17
    assert accuracy(65537, [1.0]) == -1
    assert accuracy(0, [1.0]) == -1
    assert accuracy(10, [1.0, 1.0]) == -1 and accuracy(10, [2.0, 1.0]) == -1       # not increasing
    assert accuracy(10, [1.0, float("nan")]) == -1 and accuracy(10, [float("nan")]) == -1
    assert accuracy(10, [-1.0]) == -1
