"""The evaluation leg at its chunk boundaries: balf_repeatability / balf_repeatability_batch,
balf_common_points_batch / balf_common_points_index_batch, balf_match_accuracy_batch, balf_resize_repeatability_batch and
balf_val_points (include/balf_hip.h) against the float64 NumPy references of tests/evaluation_common.py, with list lengths,
pair counts and K just before, on and just past the chunk sizes of the kernels.  Where a batched and a one-pair entry share
repeat_core.h the two are also compared bit for bit.  tests/test_evaluation_edges_host.py pins the references and the
properties of the inputs."""
import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd._lib import BalfHipError
from balf_amd.benchmark_test import evaluate, repeatability_tools as R
from oracle import oracle as O
from tests import evaluation_common as E
from tests import resize_repeat_common as RR
from tests.test_guard_gpu import GUARD, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_FIELDS = ("num_points_single_scale", "num_points_multi_scale", "possible_matches", "total_num_points")
FLOAT_FIELDS = ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale")
SCALES = ("single_scale", "multi_scale")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)       # (a copy: the shared inputs are read-only)


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in res._fields}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _packed(pairs, seed):
    rng = np.random.default_rng(seed)
    src, ns = E.pack([a for a, _ in pairs], max(len(a) for a, _ in pairs), rng)
    dst, nd = E.pack([b for _, b in pairs], max(len(b) for _, b in pairs), rng)
    return src, ns, dst, nd


def _batch(pairs, seed=1, **kw):
    src, ns, dst, nd = _packed(pairs, seed)
    return _host(R.compute_repeatability_batch(_dev(src), _dev(ns), _dev(dst), _dev(nd), **kw))


def _as_oracle(got, p, ref, what):
    """Pair p of a batched result against the oracle's dict: counts equal, floats within 1e-12 (NaN = NaN)."""
    for k in INT_FIELDS:
        assert int(got[k][p]) == int(ref[k]), (what, p, k, got[k][p], ref[k])
    for k in FLOAT_FIELDS:
        a, b = float(got[k][p]), float(ref[k])
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) < 1e-12, (what, p, k, a, b)


def _as_single(got, p, one, what):
    """... and against the one-pair entry's dict, bit for bit."""
    for k in INT_FIELDS + FLOAT_FIELDS:
        a, b = np.asarray(got[k][p]), np.asarray(one[k], dtype=got[k].dtype)
        assert np.array_equal(a, b, equal_nan=True), (what, p, k, a, b)


def _single_as_oracle(res, ref, what):
    for k in INT_FIELDS + ("correspondences", "correspondences_m"):
        assert np.array_equal(np.asarray(res[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)), (what, k)
    for k in FLOAT_FIELDS:
        assert abs(float(res[k]) - float(ref[k])) < 1e-12, (what, k)


def _one_pair(src, dst):
    with np.errstate(invalid="ignore", divide="ignore"):
        return R.compute_repeatability(src, dst)


# ---- 1. the row scan across its 1024-row chunks -----------------------------------------------------------------------------
def test_row_scan_carries_across_chunks():
    """ns = 1023, 1024, 1025, 2049 (and the transpose 3 x 2049) in ONE call, garbage past every count: per pair the oracle's
    result, the one-pair entry's bits, and the reference's candidate counts."""
    pairs = E.row_scan_pairs()
    got = _batch(pairs)
    for p, (src, dst) in enumerate(pairs):
        _as_oracle(got, p, E.oracle_repeatability(src, dst), "row scan")
        _as_single(got, p, _one_pair(src, dst), "row scan")
        _, totals = E.candidate_counts(src, dst)
        assert (int(got["candidates_single_scale"][p]), int(got["candidates_multi_scale"][p])) == tuple(totals), p


# ---- 2. the pair scan across its 1024-pair chunks ---------------------------------------------------------------------------
def test_pair_scan_carries_across_chunks():
    """P = 2050 small pairs, empty sides among them: per pair the oracle's result and the reference's candidate counts; the
    permuted batch gives the permuted results, bit for bit."""
    pairs = E.pair_scan_pairs()
    src, ns, dst, nd = _packed(pairs, 2)
    assert src.shape[1] == dst.shape[1] == E.PAIR_SCAN_N
    got = _host(R.compute_repeatability_batch(_dev(src), _dev(ns), _dev(dst), _dev(nd)))
    for p, (a, b) in enumerate(pairs):
        _as_oracle(got, p, E.oracle_repeatability(a, b), "pair scan")
        _, totals = E.candidate_counts(a, b)
        assert (int(got["candidates_single_scale"][p]), int(got["candidates_multi_scale"][p])) == tuple(totals), p
    perm = np.random.default_rng(22).permutation(len(pairs))
    again = _host(R.compute_repeatability_batch(_dev(src[perm]), _dev(ns[perm]), _dev(dst[perm]), _dev(nd[perm])))
    for k in got:
        assert np.array_equal(again[k], got[k][perm], equal_nan=True), k


# ---- 3. the exact overflow boundary -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_overflow_boundary_is_exact(which):
    """max_edges == the cumulative end of pair j's slice: pair j fits.  One lower: exactly pair j and the later pairs of that
    scale report -1 / NaN; everything that still fits has the bits of the unconstrained run."""
    pairs, j = E.overflow_pairs(), 3
    free = _batch(pairs)
    cand = np.stack([free["candidates_single_scale"], free["candidates_multi_scale"]], axis=1).astype(np.int64)
    for p, (a, b) in enumerate(pairs):
        assert tuple(cand[p]) == tuple(E.candidate_counts(a, b)[1]), p
    end = np.cumsum(cand, axis=0)
    assert cand[j, which] > 0
    for max_edges, first_over in ((int(end[j, which]), j + 1), (int(end[j, which]) - 1, j)):
        got = _batch(pairs, max_edges=max_edges)
        for w, name in enumerate(SCALES):
            over = end[:, w] > max_edges
            if w == which:
                assert np.array_equal(over, np.arange(len(pairs)) >= first_over)
            assert np.array_equal(got[f"num_points_{name}"] == -1, over), (max_edges, name)
            assert np.isnan(got[f"rep_{name}"][over]).all() and np.isnan(got[f"error_overlap_{name}"][over]).all()
            for k in (f"num_points_{name}", f"rep_{name}", f"error_overlap_{name}"):
                assert np.array_equal(got[k][~over], free[k][~over], equal_nan=True), (max_edges, k)
            assert np.array_equal(got[f"candidates_{name}"], free[f"candidates_{name}"])
        for k in ("possible_matches", "total_num_points"):
            assert np.array_equal(got[k], free[k])


def test_one_pair_overflow_boundary_is_exact(monkeypatch):
    src, dst = E.overflow_pairs()[2]
    need = int(E.candidate_counts(src, dst)[1].max())
    assert need < len(src) * len(dst)
    free = _one_pair(src, dst)
    monkeypatch.setattr(R, "MAX_EDGES", need)
    _single_as_oracle(_one_pair(src, dst), free, "MAX_EDGES == the candidate count")
    monkeypatch.setattr(R, "MAX_EDGES", need - 1)
    with pytest.raises(BalfHipError, match="candidate pairs"):
        _one_pair(src, dst)


# ---- 4. the sort and the greedy walk ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", E.EQUAL_KEY_SHAPES)
def test_equal_keys_keep_flat_index_order(a, b):
    """Every key equal: every pass of the sort is skipped and the list is copied across; flat-index order survives, so the
    assignments are exactly (k, k)."""
    src, dst = E.equal_key_pair(a, b)
    got = _one_pair(src, dst)
    want = np.stack([np.arange(min(a, b)), np.arange(min(a, b))], axis=1)
    assert np.array_equal(got["correspondences"], want) and np.array_equal(got["correspondences_m"], want)
    _single_as_oracle(got, E.oracle_repeatability(src, dst), (a, b))


def test_few_valued_keys_sort_stably():
    for case in E.FEW_KEY_CASES:
        src, dst = E.few_key_pair(case)
        _single_as_oracle(_one_pair(src, dst), E.oracle_repeatability(src, dst), case[:2])


@pytest.mark.parametrize("ns", E.WORD_EDGES)
def test_visited_bitmaps_at_word_edges(ns):
    for nd in E.WORD_EDGES:
        src, dst = E.word_edge_pair(ns, nd)
        _single_as_oracle(_one_pair(src, dst), E.oracle_repeatability(src, dst), (ns, nd))


@pytest.mark.parametrize("long_side", [0, 1])
def test_longest_lists(long_side):
    """65536 rows on one side, batched and one-pair, against the oracle."""
    src, dst = E.limit_pair(long_side)
    ref = E.oracle_repeatability(src, dst)
    one = _one_pair(src, dst)
    _single_as_oracle(one, ref, long_side)
    got = _batch([(src, dst)])
    _as_oracle(got, 0, ref, "limit")
    _as_single(got, 0, one, "limit")
    assert (int(got["candidates_single_scale"][0]), int(got["candidates_multi_scale"][0])) == tuple(E.candidate_counts(src, dst)[1])


# ---- 5. the common-region filter --------------------------------------------------------------------------------------------
def _common_inputs(cases_, seed=5):
    rng = np.random.default_rng(seed)
    n_max = max(max(len(c["src"]), len(c["dst"])) for c in cases_)
    src, _ = E.pack([c["src"] for c in cases_], n_max, rng)
    dst, _ = E.pack([c["dst"] for c in cases_], n_max, rng)
    ns, nd = (np.asarray([c[k] for c in cases_], np.int32) for k in ("ns", "nd"))
    return src, ns, dst, nd, np.stack([c["h"] for c in cases_]), np.asarray([c["shapes"] for c in cases_], np.int32)


def _check_common(cases_, out, n_max):
    cs, cd, kept, valid, i_s, i_d = out
    for p, c in enumerate(cases_):
        rows_s, rows_d = c["src"][:int(np.clip(c["ns"], 0, n_max))], c["dst"][:int(np.clip(c["nd"], 0, n_max))]
        ks, kd, want_s, want_d = E.common_points_ref(rows_s, rows_d, c["h"], c["shapes"])
        name = c["name"]
        assert tuple(kept[p]) == (len(ks), len(kd)), (name, kept[p], len(ks), len(kd))
        assert bool(valid[p]) == (len(ks) > 0 and len(kd) > 0), name
        assert np.array_equal(_bits(cs[p, :len(ks)]), _bits(ks)), name
        assert not cs[p, len(ks):].any() and not cd[p, len(kd):].any(), name
        assert np.array_equal(_bits(cd[p, :len(kd), 3]), _bits(kd[:, 3])), name
        assert len(kd) == 0 or np.abs(cd[p, :len(kd), :3] - kd[:, :3]).max() < 1e-12, name
        if i_s is not None:
            assert np.array_equal(i_s[p, :len(ks)], want_s) and (i_s[p, len(ks):] == -1).all(), name
            assert np.array_equal(i_d[p, :len(kd)], want_d) and (i_d[p, len(kd):] == -1).all(), name


def test_common_region_filter_edges():
    """Every case of part 5 in ONE batch (a bad pair must not disturb its neighbours), through both entries: kept rows, their
    order and indices bit-equal to the reference, the warped destination rows within 1e-12, zeros and -1 past the counts."""
    cases_ = E.common_cases()
    src, ns, dst, nd, h, shapes = _common_inputs(cases_)
    assert src.shape[1] == E.COMMON_N_MAX
    args = (_dev(src), _dev(ns), _dev(dst), _dev(nd), _dev(h), _dev(shapes))
    plain = [t.cpu().numpy() for t in evaluate.common_points_batch(*args)]
    index = [t.cpu().numpy() for t in evaluate.common_points_index_batch(*args)]
    for a, b in zip(plain, index[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))    # the four shared outputs: the same bits
    _check_common(cases_, index, E.COMMON_N_MAX)
    by_name = {c["name"]: p for p, c in enumerate(cases_)}
    kept = index[2]
    for n in ("inside_255_513", "inside_256_257", "inside_257_256", "inside_513_255"):       # all inside: order kept
        p = by_name[n]
        assert tuple(kept[p]) == (len(cases_[p]["src"]), len(cases_[p]["dst"]))
        assert np.array_equal(index[4][p, :kept[p, 0]], np.arange(kept[p, 0]))
    assert tuple(kept[by_name["counts_clamped"]]) == (0, E.COMMON_N_MAX)
    for n in ("30x30", "singular", "zero_shape", "negative_shape"):
        assert tuple(kept[by_name[n]]) == (0, 0) and index[3][by_name[n]] == 0
    assert kept[by_name["one_side_empty"], 0] == 0 and kept[by_name["one_side_empty"], 1] == 80


# ---- 6. the match verification ----------------------------------------------------------------------------------------------
def _accuracy_raw(c, thresholds, n_calls=1):
    """balf_match_accuracy_batch through ctypes over pre-filled outputs -> (err, correct)."""
    p, cap = c["match_idx"].shape[:2]
    t = [_dev(c[k]) for k in ("src", "dst", "kept", "match_idx", "match_count")]
    err = torch.full((p, cap), 7.25, dtype=torch.float64, device=DEV)
    correct = torch.full((p, len(thresholds)), -77, dtype=torch.int32, device=DEV)
    arr = (_lib.C.c_double * len(thresholds))(*thresholds)
    for _ in range(n_calls):
        rc = _lib.lib().balf_match_accuracy_batch(t[0].data_ptr(), E.MATCH_N_MAX, t[1].data_ptr(), E.MATCH_N_MAX, t[2].data_ptr(),
                                                  t[3].data_ptr(), t[4].data_ptr(), cap, p, arr, len(thresholds), err.data_ptr(),
                                                  correct.data_ptr(), _stream())
        assert rc == 0
    torch.cuda.synchronize()
    return err.cpu().numpy(), correct.cpu().numpy()


def _same_errors(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("cap", E.MATCH_CAPS)
def test_match_accuracy_edges(cap):
    """cap around the 256-thread stride, T = 1 and T = 16, thresholds AT the exact errors 5, 10, 13 (inclusive) and one float
    below (exclusive), bad indices, clamped counts: err bit-equal to np.sqrt(dx*dx + dy*dy) (NaN where the reference has
    NaN), correct equal, every slot written over the pre-fill; the Python layer gives the same."""
    c = E.match_case(cap)
    for ths in (E.THRESHOLDS_16,) + E.THRESHOLDS_1:
        want_err, want_correct = E.match_accuracy_np(c["src"], c["dst"], c["kept"], c["match_idx"], c["match_count"], ths)
        err, correct = _accuracy_raw(c, ths)
        assert _same_errors(err, want_err), (cap, len(ths))
        assert np.array_equal(correct, want_correct), (cap, len(ths), correct, want_correct)
    err_py, correct_py = evaluate.match_accuracy_batch(*(_dev(c[k]) for k in ("src", "dst", "kept", "match_idx", "match_count")),
                                                       E.THRESHOLDS_1[1])
    assert _same_errors(err_py.cpu().numpy(), want_err) and np.array_equal(correct_py.cpu().numpy(), want_correct)


# ---- 7. the resize protocol beyond one LDS tile -----------------------------------------------------------------------------
def _resize_batch(srcs, dsts, h, shapes, k, thr):
    ns_max, nd_max = max(map(len, srcs)), max(map(len, dsts))
    src, dst = np.full((len(srcs), ns_max, 3), np.nan), np.full((len(srcs), nd_max, 3), np.nan)
    for i, (a, b) in enumerate(zip(srcs, dsts)):
        src[i, :len(a)], dst[i, :len(b)] = a, b
    r = R.compute_resize_repeatability_batch(_dev(src), _dev(np.asarray([len(a) for a in srcs], np.int32)), _dev(dst),
                                             _dev(np.asarray([len(b) for b in dsts], np.int32)), h, shapes, k, thr)
    return {f: getattr(r, f).cpu().numpy() for f in r._fields}


def _as_resize_reference(got, want, what):
    """Counts equal, repeatability bit-equal, localization_err within 1e-9.  Derived as in test_golden_cases_one_pair, for
    these inputs: coordinates are below 2^12, a warp is about ten float64 operations (<= ~4e-12 per coordinate), a distance
    inherits about twice that (<= ~1e-11), and a mean of <= 2 x 3000 terms <= 3 adds <= 6000 * 2^-53 * 3 = 2e-12 for the order
    of summation: < 2e-11 in all, so 1e-9 leaves a factor 50."""
    for key in RR.KEYS[2:]:
        assert int(got[key]) == int(want[key]), (what, key, got[key], want[key])
    assert np.float64(got["repeatability"]) == np.float64(want["repeatability"]), what
    assert abs(float(got["localization_err"]) - float(want["localization_err"])) < 1e-9, what


@pytest.mark.parametrize("case", E.RESIZE_CASES)
def test_resize_minima_beyond_one_tile(case):
    """K = 1024, 1025, 2049, 3000 kept rows on one side (n above K) against fewer than K on the other, both ways round: the
    nearest neighbours sit in every LDS tile and at the last column of a partial tile.  One pair, and a batch of P = 3 with
    unequal counts whose pairs carry the one-pair bits."""
    k = case[0]
    shape = E.RESIZE_SHAPE
    pairs = [E.resize_case(*case, True), E.resize_case(*case, False)]
    wants = [E.resize_case_reference(*case, True)[0], E.resize_case_reference(*case, False)[0]]
    pairs.append((pairs[0][0][:700], pairs[0][1][:650]))
    wants.append(RR.resize_repeatability_np(*pairs[2], E.RESIZE_H, shape, shape, k, E.RESIZE_THRESH)[0])
    ones = []
    for (src, dst), want in zip(pairs[:2], wants[:2]):
        one = R.compute_resize_repeatability(src.copy(), dst.copy(), E.RESIZE_H, shape, shape, k, E.RESIZE_THRESH)
        _as_resize_reference(one, want, ("one pair", case))
        ones.append(one)
    got = _resize_batch([a for a, _ in pairs], [b for _, b in pairs], np.stack([E.RESIZE_H] * 3),
                        np.tile(np.asarray(shape + shape, np.int32), (3, 1)), k, E.RESIZE_THRESH)
    for p, want in enumerate(wants):
        _as_resize_reference({f: got[f][p] for f in RR.KEYS}, want, ("batch", case, p))
    for p, one in enumerate(ones):
        for f in RR.KEYS:
            assert np.array_equal(np.asarray(got[f][p], np.float64), np.asarray(one[f], np.float64)), (case, p, f)


def test_signed_zero_probs_tie_at_the_cut():
    """The cut falls between rows of prob -0.0 (lower indices) and +0.0, on both sides: the two are EQUAL probs, so the lower
    index is kept (NumPy's and the restatement's order)."""
    src, dst, h, ss, sd, k, thr = E.signed_zero_case()
    want, _, _ = RR.resize_repeatability_np(src, dst, h, ss, sd, k, thr)
    got = R.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    print({key: (float(got[key]), float(want[key])) for key in RR.KEYS})
    _as_resize_reference(got, want, "signed zero")
    assert int(got["rep_src_num"]) == int(got["rep_dst_num"]) == 20


# ---- 8. the validation selection at large K ---------------------------------------------------------------------------------
VAL_RUNS = [(shapes, k) for shapes in E.VAL_SHAPES for k in E.VAL_KS if k <= min(s[0] * s[1] for s in shapes)]


@pytest.mark.parametrize("leg,nms_size", E.VAL_LEGS)
def test_val_selection_at_large_k(leg, nms_size):
    """K from 1 to the documented maximum 16384 (= H * W of the 128 x 128 maps; 6000 is the first K whose sort needs more
    than 48 KB of LDS), P = 3 pairs with a homography each, dense / 8-level / sparse / all-zero maps and a homography without
    a common region: counts equal, source rows bit-equal to get_point_coordinates on the oracle's masked NMS map, zero rows
    past the count; warped destination rows: score bit-equal, position and radius within 1e-12 of apply_homography_to_points
    (the bar of test_selection_on_recorded_maps_is_the_references)."""
    assert (E.VAL_SHAPES[0], 16384) in VAL_RUNS and len(VAL_RUNS) == 13
    full, short, fallback = 0, 0, 0
    for shapes, k in VAL_RUNS:
        for batch in range(len(E.VAL_BATCHES)):
            ps, pd, hs = E.val_batch(batch, shapes)
            masked = E.val_masked_maps(batch, shapes, leg, nms_size)
            src, dst, count = (t.cpu().numpy() for t in ops.val_points(_dev(ps), _dev(pd), _dev(hs), nms_size, k, leg))
            for p in range(len(hs)):
                want_s, want_d = E.val_select(masked[p][0], k), E.val_select(masked[p][1], k)
                what = (leg, nms_size, shapes, k, batch, p)
                assert tuple(count[p]) == (len(want_s), len(want_d)), (what, count[p], len(want_s), len(want_d))
                assert np.array_equal(_bits(src[p, :len(want_s)]), _bits(want_s)), what
                assert not src[p, len(want_s):].any() and not dst[p, len(want_d):].any(), what
                want_w = O.apply_homography_to_points(want_d, hs[p])
                got_w = dst[p, :len(want_d)]
                assert np.array_equal(_bits(got_w[:, 3]), _bits(want_w[:, 3])), what
                assert np.abs(got_w[:, :3] - want_w[:, :3]).max() < 1e-12, what
                zero = not masked[p][0].any()
                fallback += zero
                full += (not zero) and len(want_s) == k
                short += len(want_s) < k
    assert full > 10 and short > 10 and fallback > 10


# ---- 9. guard bands of this leg's C ABI -------------------------------------------------------------------------------------
def _guarded(a):
    """A host array in a device buffer of exactly its size between two guard bands."""
    a = np.ascontiguousarray(a)
    g = Guarded(a.nbytes)
    g.full[GUARD:GUARD + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(DEV)
    return g


def _broken(bufs):
    return [name for name, g in bufs.items() if not g.intact()]


def test_repeatability_batch_abi_stays_inside_its_buffers():
    l = _lib.lib()
    pairs = E.overflow_pairs()
    src, ns, dst, nd = _packed(pairs, 9)
    want = _host(R.compute_repeatability_batch(_dev(src), _dev(ns), _dev(dst), _dev(nd), max_edges=1000))
    p, ns_max, nd_max, max_edges = len(pairs), src.shape[1], dst.shape[1], 1000
    nbytes = l.balf_repeatability_batch_workspace_bytes(p, ns_max, nd_max, max_edges)
    assert nbytes > 0
    b = dict(src=_guarded(src), ns=_guarded(ns), dst=_guarded(dst), nd=_guarded(nd), rep=Guarded(p * 4 * 8, fill=0x7B),
             counts=Guarded(p * 6 * 4, fill=0x7B), ws=Guarded(nbytes, fill=0xFF))

    def call(ws_bytes):
        return l.balf_repeatability_batch(b["src"].ptr, b["ns"].ptr, ns_max, 4, b["dst"].ptr, b["nd"].ptr, nd_max, 4, 1, p, 0.4,
                                          1e-6, 3.0, 30.0, max_edges, b["rep"].ptr, b["counts"].ptr, b["ws"].ptr, ws_bytes, _stream())

    for _ in range(2):                                               # the second call finds the first one's workspace
        assert call(nbytes) == 0
        torch.cuda.synchronize()
        assert _broken(b) == []
        rep = b["rep"].view(torch.float64, (p, 4)).cpu().numpy()
        cnt = b["counts"].view(torch.int32, (p, 6)).cpu().numpy()
        for col, k in enumerate(FLOAT_FIELDS):
            assert np.array_equal(rep[:, col], want[k], equal_nan=True), k
        for col, k in enumerate(INT_FIELDS + ("candidates_single_scale", "candidates_multi_scale")):
            assert np.array_equal(cnt[:, col], want[k]), k
    assert (want["num_points_multi_scale"] > 0).all() and (want["num_points_single_scale"] > 0).all()
    assert call(nbytes - 1) == -3                                    # BALF_ERR_WORKSPACE


@pytest.mark.parametrize("with_index", [False, True])
def test_common_points_abi_stays_inside_its_buffers(with_index):
    l = _lib.lib()
    cases_ = [c for c in E.common_cases() if c["name"] in ("31x31", "bad_coordinates", "perspective", "one_side_empty", "singular")]
    src, ns, dst, nd, h, shapes = _common_inputs(cases_, seed=6)
    p, n_max = len(cases_), src.shape[1]
    want = [t.cpu().numpy() for t in evaluate.common_points_index_batch(_dev(src), _dev(ns), _dev(dst), _dev(nd), _dev(h), _dev(shapes))]
    b = dict(src=_guarded(src), ns=_guarded(ns), dst=_guarded(dst), nd=_guarded(nd), h=_guarded(h), shapes=_guarded(shapes),
             src_out=Guarded(p * n_max * 32, fill=0x7B), dst_out=Guarded(p * n_max * 32, fill=0x7B),
             kept=Guarded(p * 8, fill=0x7B), valid=Guarded(p * 4, fill=0x7B))
    if with_index:
        b.update(src_index=Guarded(p * n_max * 4, fill=0x7B), dst_index=Guarded(p * n_max * 4, fill=0x7B))
    head = (b["src"].ptr, b["ns"].ptr, n_max, b["dst"].ptr, b["nd"].ptr, n_max, p, b["h"].ptr, b["shapes"].ptr, b["src_out"].ptr,
            b["dst_out"].ptr, b["kept"].ptr, b["valid"].ptr)
    for _ in range(2):
        if with_index:
            assert l.balf_common_points_index_batch(*head, b["src_index"].ptr, b["dst_index"].ptr, _stream()) == 0
        else:
            assert l.balf_common_points_batch(*head, _stream()) == 0
        torch.cuda.synchronize()
        assert _broken(b) == []
        got = [b["src_out"].view(torch.float64, (p, n_max, 4)), b["dst_out"].view(torch.float64, (p, n_max, 4)),
               b["kept"].view(torch.int32, (p, 2)), b["valid"].view(torch.int32, (p,))]
        if with_index:
            got += [b["src_index"].view(torch.int32, (p, n_max)), b["dst_index"].view(torch.int32, (p, n_max))]
        for a, w in zip(got, want):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), w.view(np.uint8))


def test_match_accuracy_abi_stays_inside_its_buffers():
    l = _lib.lib()
    c = E.match_case(257)
    ths = E.THRESHOLDS_16
    p, cap = c["match_idx"].shape[:2]
    want_err, want_correct = (t.cpu().numpy() for t in evaluate.match_accuracy_batch(
        *(_dev(c[k]) for k in ("src", "dst", "kept", "match_idx", "match_count")), ths))
    b = {k: _guarded(c[k]) for k in ("src", "dst", "kept", "match_idx", "match_count")}
    b.update(err=Guarded(p * cap * 8, fill=0x7B), correct=Guarded(p * len(ths) * 4, fill=0x7B))
    arr = (_lib.C.c_double * len(ths))(*ths)
    for _ in range(2):
        assert l.balf_match_accuracy_batch(b["src"].ptr, E.MATCH_N_MAX, b["dst"].ptr, E.MATCH_N_MAX, b["kept"].ptr,
                                           b["match_idx"].ptr, b["match_count"].ptr, cap, p, arr, len(ths), b["err"].ptr,
                                           b["correct"].ptr, _stream()) == 0
        torch.cuda.synchronize()
        assert _broken(b) == []
        assert _same_errors(b["err"].view(torch.float64, (p, cap)).cpu().numpy(), want_err)
        assert np.array_equal(b["correct"].view(torch.int32, (p, len(ths))).cpu().numpy(), want_correct)
