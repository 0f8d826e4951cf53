"""The matching-score leg of the HSequences evaluation on the GPU (balf_common_points_index_batch / balf_match_accuracy_batch in
include/balf_hip.h; evaluate.evaluate_matching_pairs / evaluate_matching_hsequences) against balf_common_points_batch and the
NumPy restatement of DESIGN.md 7h (tests/matching_common.py)."""
import ctypes

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch
from balf_amd.benchmark_test import _chunked, evaluate
from balf_amd.model import get_model
from balf_amd.third_party.hardnet.hardnet_pytorch import HardNet
from balf_amd.utils import synth
from tests import matching_common as MC
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _stream():
    return _lib.current_stream_ptr(torch.device(DEV))


# ---- 1. keep-index ------------------------------------------------------------------------------------------------------------
def _index_inputs():
    """P = 4 pairs of 96x128 / 80x112 images, about 40 integer-pixel rows a side: a translated pair, a pair whose destination
    rows all lie outside the common region, a singular homography, a pair whose source count is 0."""
    rng = np.random.default_rng(11)
    hs, ws, hd, wd = 96, 128, 80, 112
    n_s, n_d, ns_max, nd_max = 41, 39, 45, 43

    def rows(h, w, n, x_hi=None):
        return np.stack([rng.integers(0, x_hi or w, n), rng.integers(0, h, n), rng.choice([1.0, 2.0], n),
                         rng.uniform(0, 1, n)], axis=1).astype(np.float64)

    shift = np.array([[1.0, 0.0, 6.0], [0.0, 1.0, 4.0], [0.0, 0.0, 1.0]])
    src = rng.uniform(-1e4, 1e4, (4, ns_max, 4))
    dst = rng.uniform(-1e4, 1e4, (4, nd_max, 4))
    for p in range(4):
        src[p, :n_s] = rows(hs, ws, n_s)
        dst[p, :n_d] = rows(hd, wd, n_d, x_hi=12 if p == 1 else None)      # pair 1: x < 12, inside the 15-pixel frame
    h = np.stack([shift, shift, np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]), shift])
    ns = np.array([n_s, n_s, n_s, 0], dtype=np.int32)
    nd = np.array([n_d, n_d, n_d, n_d], dtype=np.int32)
    shapes = np.array([[hs, ws, hd, wd]] * 4, dtype=np.int32)
    return src, ns, dst, nd, h, shapes


def test_keep_index_equals_the_filter_and_names_the_rows():
    src, ns, dst, nd, h, shapes = _index_inputs()
    t = [torch.from_numpy(a).to(DEV) for a in (src, ns, dst, nd, h, shapes)]
    ref = evaluate.common_points_batch(*t)
    p, ns_max, nd_max = src.shape[0], src.shape[1], dst.shape[1]
    # the library called on buffers pre-filled with a sentinel: every slot must be written
    out_s = torch.full((p, ns_max, 4), 777.0, dtype=torch.float64, device=DEV)
    out_d = torch.full((p, nd_max, 4), 777.0, dtype=torch.float64, device=DEV)
    kept = torch.full((p, 2), -7, dtype=torch.int32, device=DEV)
    valid = torch.full((p,), -7, dtype=torch.int32, device=DEV)
    idx_s = torch.full((p, ns_max), -7, dtype=torch.int32, device=DEV)
    idx_d = torch.full((p, nd_max), -7, dtype=torch.int32, device=DEV)
    rc = _lib.lib().balf_common_points_index_batch(t[0].data_ptr(), t[1].data_ptr(), ns_max, t[2].data_ptr(), t[3].data_ptr(),
                                                   nd_max, p, t[4].data_ptr(), t[5].data_ptr(), out_s.data_ptr(),
                                                   out_d.data_ptr(), kept.data_ptr(), valid.data_ptr(), idx_s.data_ptr(),
                                                   idx_d.data_ptr(), _stream())
    assert rc == 0
    got = evaluate.common_points_index_batch(*t)
    torch.cuda.synchronize()
    for a, b, c in zip((out_s, out_d, kept, valid), ref, got[:4]):
        a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
        if a.dtype == np.float64:
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(c), _bits(b))
        else:
            assert np.array_equal(a, b) and np.array_equal(c, b)
    assert torch.equal(got.src_index, idx_s) and torch.equal(got.dst_index, idx_d)
    kept, valid, idx_s, idx_d = kept.cpu().numpy(), valid.cpu().numpy(), idx_s.cpu().numpy(), idx_d.cpu().numpy()
    out_s, out_d = out_s.cpu().numpy(), out_d.cpu().numpy()
    assert kept[0, 0] > 5 and kept[0, 1] > 5 and valid[0] == 1       # the translated pair keeps rows on both sides, not all
    assert kept[0, 0] < ns[0] and kept[0, 1] < nd[0]
    assert kept[1, 0] > 0 and kept[1, 1] == 0 and valid[1] == 0      # destination wholly outside
    assert kept[2].tolist() == [0, 0] and valid[2] == 0              # singular
    assert kept[3, 0] == 0 and kept[3, 1] > 0 and valid[3] == 0      # count 0
    for q in range(p):
        for index, k, n in ((idx_s[q], kept[q, 0], ns[q]), (idx_d[q], kept[q, 1], nd[q])):
            assert (index[k:] == -1).all()
            assert (np.diff(index[:k]) > 0).all() and (index[:k] >= 0).all() and (index[:k] < n).all()
        k = kept[q, 0]
        assert np.array_equal(_bits(out_s[q, :k]), _bits(src[q, idx_s[q, :k]]))
        k = kept[q, 1]                                                # the warp carries the score: column 3 names the row
        assert np.array_equal(_bits(out_d[q, :k, 3]), _bits(dst[q, idx_d[q, :k], 3]))
        r = MC.kept_lists(src[q, :ns[q]], dst[q, :nd[q]], h[q], shapes[q, :2], shapes[q, 2:])
        assert np.array_equal(r[2], idx_s[q, :kept[q, 0]]) and np.array_equal(r[3], idx_d[q, :kept[q, 1]])


# ---- 2. match accuracy ----------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 300)       # around one wave, and beyond one pass of the 256-thread block
CAP, NS_MAX, ND_MAX = 320, 330, 340


def _accuracy_inputs(seed):
    rng = np.random.default_rng(seed)
    p = len(COUNTS)
    src = np.concatenate([rng.uniform(0, 4096, (p, NS_MAX, 2)), rng.uniform(0, 2, (p, NS_MAX, 2))], axis=2)
    dst = np.concatenate([rng.uniform(0, 4096, (p, ND_MAX, 2)), rng.uniform(0, 2, (p, ND_MAX, 2))], axis=2)
    kept = np.stack([rng.integers(CAP, NS_MAX + 1, p), rng.integers(CAP, ND_MAX + 1, p)], axis=1).astype(np.int32)
    midx = np.full((p, CAP, 2), -1, dtype=np.int32)
    for q, m in enumerate(COUNTS):
        i, j = rng.permutation(kept[q, 0])[:m], rng.permutation(kept[q, 1])[:m]
        midx[q, :m, 0], midx[q, :m, 1] = i, j
        r, a = rng.uniform(0, 12, m), rng.uniform(0, 2 * np.pi, m)    # errors spread over and past the thresholds
        dst[q, j, 0] = np.clip(src[q, i, 0] + r * np.cos(a), 0, 4095.5)
        dst[q, j, 1] = np.clip(src[q, i, 1] + r * np.sin(a), 0, 4095.5)
    q = len(COUNTS) - 1                                               # planted: indices outside [0, kept) inside the count
    midx[q, 7] = (kept[q, 0], 3)
    midx[q, 100] = (5, -1)
    midx[q, 299] = (1 << 30, 0)
    midx[q, 150] = (2, kept[q, 1])
    return src, dst, kept, midx, np.asarray(COUNTS, dtype=np.int32)


def _decided_inputs(thresholds):
    """Inputs where no error lies within 1e-9 of a threshold, so that the restatement alone decides every count: checked here,
    on the CPU; the next seed is drawn otherwise."""
    for seed in range(100, 120):
        src, dst, kept, midx, count = _accuracy_inputs(seed)
        errs = [MC.reprojection_errors(src[q, :kept[q, 0]], dst[q, :kept[q, 1]], midx[q, :count[q]]) for q in range(len(count))]
        e = np.concatenate(errs)
        e = e[~np.isnan(e)]
        if np.abs(e[:, None] - np.asarray(thresholds, dtype=np.float64)[None, :]).min() > 1e-9:
            return src, dst, kept, midx, count, errs
    raise AssertionError("no seed gave errors clear of the thresholds")


@pytest.fixture(scope="module")
def accuracy_case():
    return _decided_inputs(range(1, 11))


@pytest.mark.parametrize("thresholds", [list(range(1, 11)), [3]], ids=["T10", "T1"])
def test_match_accuracy_equals_the_restatement(accuracy_case, thresholds):
    src, dst, kept, midx, count, errs = accuracy_case
    p, t_n = len(count), len(thresholds)
    t = [torch.from_numpy(a).to(DEV) for a in (src, dst, kept, midx, count)]
    err = torch.full((p, CAP), 777.0, dtype=torch.float64, device=DEV)
    correct = torch.full((p, t_n), -7, dtype=torch.int32, device=DEV)
    th = (ctypes.c_double * t_n)(*[float(v) for v in thresholds])
    rc = _lib.lib().balf_match_accuracy_batch(t[0].data_ptr(), NS_MAX, t[1].data_ptr(), ND_MAX, t[2].data_ptr(), t[3].data_ptr(),
                                              t[4].data_ptr(), CAP, p, th, t_n, err.data_ptr(), correct.data_ptr(), _stream())
    assert rc == 0
    err2, correct2 = evaluate.match_accuracy_batch(*t, thresholds)
    torch.cuda.synchronize()
    assert torch.equal(correct, correct2) and torch.equal(err.nan_to_num(-1.0), err2.nan_to_num(-1.0))
    err, correct = err.cpu().numpy(), correct.cpu().numpy()
    n_nan = 0
    for q in range(p):
        ref = np.full(CAP, np.nan)
        ref[:count[q]] = errs[q]
        assert np.array_equal(np.isnan(err[q]), np.isnan(ref)), q                  # NaN exactly where specified
        ok = ~np.isnan(ref)
        # a handful of float64 roundings at magnitude 2^12: 2^12 * 2^-52 ~ 1e-12
        assert np.abs(err[q][ok] - ref[ok]).max(initial=0.0) <= 1e-12, q
        assert correct[q].tolist() == MC.correct_counts(errs[q], thresholds).tolist(), q
        n_nan += int(np.isnan(errs[q]).sum())
    assert n_nan == 4                                                             # the planted indices
    assert correct[-1, -1] > correct[-1, 0] > 0 or t_n == 1


# ---- 3. pairs end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(cases.WEIGHT_SEED))
    m.precision = "fp32"
    hn = HardNet()
    hn.load_state_dict(synth.synthetic_hardnet_state_dict(5))
    return m.eval().to(DEV), hn.eval().to(DEV)


def _detect_describe(images_norm, nets, num_points):
    """rows [I,K,4], count [I], desc [I,K,128] of some normalised RGB images, each detected and described once."""
    detector, descriptor = nets
    dev = torch.device(DEV)
    with torch.no_grad():
        rows, count = _chunked.detect_images(images_norm, detector, dev, 15, num_points, 15, False, 16)
        grays = [evaluate._gray_u8(None, im, dev) for im in images_norm]
        desc = _chunked.describe_images(grays, rows, count, descriptor, 60, 16)
    return rows, count, desc


REP_INT = ("num_points_single_scale", "num_points_multi_scale", "possible_matches", "total_num_points")


def _check_pair(got, q, ref, thresholds):
    """Every field of pair q against the restatement's record: integers exactly, ratios as the quotient of the exact
    integers."""
    assert (int(got["kept"][q, 0]), int(got["kept"][q, 1])) == ref["num_features"]
    assert int(got["valid"][q]) == ref["valid"]
    m = ref["num_mutual_corresp"]
    assert int(got["num_mutual_corresp"][q]) == m
    assert int(got["num_matches"][q]) == ref["num_matches"]
    assert got["correct"][q].tolist() == ref["correct"].tolist()
    assert np.array_equal(got["match_idx"][q, :m], ref["match_idx"]) and (got["match_idx"][q, m:] == -1).all()
    assert np.isnan(got["match_err"][q, m:]).all()
    assert np.abs(got["match_err"][q, :m] - ref["match_err"]).max(initial=0.0) <= 1e-12
    for k in ("mma", "mma_corr", "avg_mma"):
        assert float(got[k][q]) == ref[k], (k, float(got[k][q]), ref[k])
    rep = ref["repeatability"]
    if rep is not None:
        for k in REP_INT:
            assert int(got[k][q]) == int(rep[k]), k
        for k in ("rep_single_scale", "rep_multi_scale"):              # found / total * 100: the quotient of the integers
            assert float(got[k][q]) == float(rep[k]), k
        for k in ("error_overlap_single_scale", "error_overlap_multi_scale"):
            assert abs(float(got[k][q]) - float(rep[k])) < 1e-12, k    # (the bound of the repeatability goldens)


def test_pairs_end_to_end_equal_the_restatement(nets):
    g = synth.synthetic_gray_u8(192, 256, 31)
    h, w = 128, 192
    win0 = synth.gray_to_rgb_norm(g[20:20 + h, 20:20 + w])
    win1 = synth.gray_to_rgb_norm(g[25:25 + h, 28:28 + w])               # window 0 moved by (8, 5): dst (x, y) = src (x + 8, y + 5)
    rows, count, desc = _detect_describe([win0, win1], nets, 64)
    eye = np.eye(3)
    shift = np.array([[1.0, 0.0, 8.0], [0.0, 1.0, 5.0], [0.0, 0.0, 1.0]])
    far = np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])        # the windows do not overlap
    hs = np.stack([eye, shift, far])
    s_at = torch.tensor([0, 0, 0], device=DEV)
    d_at = torch.tensor([0, 1, 1], device=DEV)
    shapes = torch.tensor([[h, w, h, w]] * 3, dtype=torch.int32, device=DEV)
    r = evaluate.evaluate_matching_pairs(rows[s_at], count[s_at], desc[s_at], rows[d_at], count[d_at], desc[d_at],
                                         torch.from_numpy(hs).to(DEV), shapes)
    got = {k: v.cpu().numpy() for k, v in r._asdict().items()}
    rows_h, count_h, desc_h = rows.cpu().numpy(), count.cpu().numpy(), desc.cpu().numpy()
    assert count_h.min() > 20
    refs = []
    for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 1))):
        ref = MC.pair_record(rows_h[i, :count_h[i]], rows_h[j, :count_h[j]], desc_h[i, :count_h[i]], desc_h[j, :count_h[j]],
                             hs[q], (h, w), (h, w))
        _check_pair(got, q, ref, range(1, 11))
        refs.append(ref)
    # the identical pair: every kept point finds itself
    ks = refs[0]["num_features"][0]
    assert ks > 20 and got["num_mutual_corresp"][0] == ks and got["mma"][0] == 1.0 and got["avg_mma"][0] == 1.0
    assert (got["match_err"][0, :ks] == 0.0).all()
    # the translated pair matches, and correctly; the third pair is not valid and scores 0
    assert refs[1]["valid"] == 1 and refs[1]["num_matches"] > 5
    assert got["valid"][2] == 0 and got["num_mutual_corresp"][2] == 0
    assert got["mma"][2] == 0.0 and got["mma_corr"][2] == 0.0 and got["avg_mma"][2] == 0.0


# ---- 4. graph capture -------------------------------------------------------------------------------------------------------------
def _nan_equal(a, b):
    if a.is_floating_point():
        a, b = a.nan_to_num(-7.0), b.nan_to_num(-7.0)
    return torch.equal(a, b)


def test_evaluate_matching_pairs_replays_in_a_graph():
    p, n = 4, 96

    def make(seed):
        r = np.random.default_rng(seed)
        src = np.stack([r.integers(0, 320, (p, n)), r.integers(0, 240, (p, n)), np.ones((p, n)), r.uniform(0, 1, (p, n))],
                       axis=2).astype(np.float64)
        hs, perms, dst = [], [], np.empty_like(src)
        for q in range(p):
            dx, dy = int(r.integers(-9, 10)), int(r.integers(-9, 10))
            hs.append(np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]]))
            perms.append(r.permutation(n))
            dst[q] = src[q, perms[q]]
            dst[q, :, 0] -= dx + r.integers(-3, 4, n)                  # up to 3 pixels off: errors on both sides of thresholds
            dst[q, :, 1] -= dy
        d_src = r.normal(0, 1, (p, n, 128)).astype(np.float32)
        d_src /= np.linalg.norm(d_src, axis=2, keepdims=True)
        d_dst = np.stack([d_src[q, perms[q]] for q in range(p)]) + r.normal(0, 0.02, (p, n, 128)).astype(np.float32)
        ns = r.integers(n // 2, n + 1, p).astype(np.int32)
        nd = r.integers(n // 2, n + 1, p).astype(np.int32)
        arrs = (src, ns, d_src, dst, nd, d_dst.astype(np.float32), np.stack(hs),
                np.array([[240, 320, 240, 320]] * p, dtype=np.int32))
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrs)

    static = make(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            evaluate.evaluate_matching_pairs(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = evaluate.evaluate_matching_pairs(*static)
    for seed in (10, 20):
        new = make(seed)
        for a, b in zip(static, new):
            a.copy_(b)
        graph.replay()
        got = {k: v.clone() for k, v in out._asdict().items()}
        ref = evaluate.evaluate_matching_pairs(*new)
        torch.cuda.synchronize()
        assert int(ref.valid.sum()) > 0 and int(ref.num_mutual_corresp.sum()) > 10
        assert int(ref.num_matches.sum()) > 0
        for k, v in ref._asdict().items():
            assert _nan_equal(got[k], v), k


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------
class _Loader:
    """Two sequences of translated windows of a synthetic image: 'a' (128 x 192) with two destinations, 'b' (112 x 160) with
    one."""

    def __init__(self):
        self.sequences = ["a", "b"]
        self._data = []
        for s, ((h, w), shifts) in enumerate((((128, 192), [(6, 3), (-4, 7)]), ((112, 160), [(5, -6)]))):
            g = synth.synthetic_gray_u8(h + 40, w + 40, 40 + s)
            dsts, hs = [], []
            for dx, dy in shifts:
                dsts.append(synth.gray_to_rgb_norm(g[20 + dy:20 + dy + h, 20 + dx:20 + dx + w]))
                hs.append(np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]]))
            self._data.append(dict(sequence_name=self.sequences[s], im_src_RGB_norm=synth.gray_to_rgb_norm(g[20:20 + h, 20:20 + w]),
                                   images_dst_RGB_norm=dsts, h_dst_2_src=hs))

    def get_sequence_data(self, i):
        return self._data[i]


def test_hsequences_driver_equals_pair_by_pair(nets):
    detector, descriptor = nets
    loader = _Loader()
    seen = []
    forward = detector.forward

    def counting(x, *a, **kw):
        seen.append(int(x.shape[0]))
        return forward(x, *a, **kw)

    detector.forward = counting
    try:
        res = evaluate.evaluate_matching_hsequences(loader, detector, descriptor, DEV, num_points=64)
        assert sum(seen) == 5                                        # once per image (2 sources + 3 destinations), not per pair (6)
        again = evaluate.evaluate_matching_hsequences(loader, detector, descriptor, DEV, num_points=64, chunk_sequences=1,
                                                      batch_size=1)
    finally:
        del detector.forward
    assert res == again
    assert res["sequences"] == ["a", "b"] and res["top_k"] == 64 and res["pixel_threshold"] == 5 and res["overlap"] == 0.6
    lists = [k for k in res if k not in ("sequences", "top_k", "overlap", "pixel_threshold")]
    assert len(lists) == 12 and all(len(res[k]) == 3 for k in lists)
    q = 0
    for sd in loader._data:
        for dst, hm in zip(sd["images_dst_RGB_norm"], sd["h_dst_2_src"]):
            src = sd["im_src_RGB_norm"]
            rows, count, desc = _detect_describe([src, dst], nets, 64)
            shapes = torch.tensor([src.shape[:2] + dst.shape[:2]], dtype=torch.int32, device=DEV)
            r = evaluate.evaluate_matching_pairs(rows[:1], count[:1], desc[:1], rows[1:], count[1:], desc[1:],
                                                 torch.from_numpy(hm[None]).to(DEV), shapes)
            assert int(r.valid[0]) == 1
            for k in lists:
                if k == "num_features":
                    assert res[k][q] == (int(r.kept[0, 0]), int(r.kept[0, 1]))
                else:
                    v = getattr(r, k)[0].item()
                    assert res[k][q] == v and type(res[k][q]) is type(v), (k, q, res[k][q], v)
            assert res["num_mutual_corresp"][q] > 5 and 0.0 < res["mma"][q] <= 1.0
            q += 1
