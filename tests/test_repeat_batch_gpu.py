"""Batched HSequences evaluation on the GPU (balf_common_points_batch / balf_repeatability_batch in include/balf_hip.h;
repeatability_tools.compute_repeatability_batch, benchmark_test.evaluate, train_utils.check_val_hsequences_repeatability)
against the goldens and against the one-pair functions, bit for bit."""
import os
import time

import numpy as np
import pytest
import torch

from balf_amd import arch, multiscale as MS, pipeline
from balf_amd.benchmark_test import evaluate, geometry_tools, repeatability_tools as R
from balf_amd.model import get_model
from balf_amd.utils import synth, train_utils
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale",
          "num_points_single_scale", "num_points_multi_scale", "possible_matches", "total_num_points")


def _pack(lists, n_max, rng, cols=4):
    """host row lists -> [P, n_max, cols] float64 on the device with garbage past each count, and the counts [P] int32."""
    p = len(lists)
    out = rng.uniform(-1e4, 1e4, (p, max(n_max, 1), cols))
    for k, a in enumerate(lists):
        if len(a):
            out[k, :len(a)] = np.asarray(a, dtype=np.float64)[:, :cols]
    return (torch.from_numpy(out[:, :n_max].copy()).to(DEV),
            torch.tensor([len(a) for a in lists], dtype=torch.int32, device=DEV))


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in res._fields}


def _same_as_single(got, p, ref):
    for k in FIELDS:
        a, b = np.asarray(got[k][p]), np.asarray(ref[k], dtype=got[k].dtype)
        assert np.array_equal(a, b, equal_nan=True), (p, k, a, b)


def test_goldens_as_one_batch():
    """The overlap parameters are per call: the cases with the default parameters go in ONE batch, each other case in its
    own."""
    g = np.load(os.path.join(HERE, "golden", "repeatability.npz"))
    names = [n for n in cases.REPEAT_CASES if not cases.REPEAT_CASES[n]["kw"]]
    groups = [names] + [[n] for n in cases.REPEAT_CASES if cases.REPEAT_CASES[n]["kw"]]
    rng = np.random.default_rng(3)
    seen = 0
    for grp in groups:
        ins = [cases.repeat_inputs(cases.REPEAT_CASES[n]) for n in grp]
        src, ns = _pack([a for a, _ in ins], max(len(a) for a, _ in ins), rng)
        dst, nd = _pack([b for _, b in ins], max(len(b) for _, b in ins), rng)
        got = _host(R.compute_repeatability_batch(src, ns, dst, nd, **cases.REPEAT_CASES[grp[0]]["kw"]))
        for p, n in enumerate(grp):
            for k in ("num_points_single_scale", "num_points_multi_scale", "total_num_points", "possible_matches"):
                assert int(got[k][p]) == int(g[f"{n}.{k}"]), (n, k)
            for k in ("rep_single_scale", "rep_multi_scale", "error_overlap_single_scale", "error_overlap_multi_scale"):
                assert abs(float(got[k][p]) - float(g[f"{n}.{k}"])) < 1e-12, (n, k)
            seen += 1
    assert seen == len(cases.REPEAT_CASES)


def _tie_grid():
    ys, xs = np.mgrid[0:12, 0:12]
    src = np.stack([xs.ravel() * 20.0, ys.ravel() * 20.0, np.ones(144), np.ones(144)], axis=1)
    dst = src.copy()
    dst[:, 0] += 6.0
    return src, dst


@pytest.mark.parametrize("seed", [0, 1])
def test_batch_equals_single_bit_for_bit(seed):
    rng = np.random.default_rng(100 + seed)
    pairs = [(np.zeros((0, 4)), cases.repeat_inputs(dict(ns=5, nd=5, seed=1, planted=3))[1]),
             (cases.repeat_inputs(dict(ns=7, nd=7, seed=2, planted=3))[0], np.zeros((0, 4))),
             cases.repeat_inputs(dict(ns=1, nd=1, seed=3, planted=1)),
             cases.repeat_inputs(dict(ns=1, nd=40, seed=4, planted=1)),
             cases.repeat_inputs(dict(ns=1000, nd=1000, seed=5, planted=700)),
             cases.repeat_inputs(dict(ns=3, nd=700, seed=6, planted=2)),
             _tie_grid()]
    while len(pairs) < 64:
        ns, nd = int(rng.integers(0, 300)), int(rng.integers(0, 300))
        pairs.append(cases.repeat_inputs(dict(ns=ns, nd=nd, seed=int(rng.integers(1 << 20)),
                                              planted=int(rng.integers(0, max(1, min(ns, nd)) + 1)))))
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    src, ns = _pack([a for a, _ in pairs], max(len(a) for a, _ in pairs), rng)
    dst, nd = _pack([b for _, b in pairs], max(len(b) for _, b in pairs), rng)
    got = _host(R.compute_repeatability_batch(src, ns, dst, nd))
    for p, (a, b) in enumerate(pairs):
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = R.compute_repeatability(a, b)
        _same_as_single(got, p, ref)
        assert got["candidates_single_scale"][p] >= got["num_points_single_scale"][p] >= 0


MASK_CASES = [
    ((240, 320), (240, 320), cases.HOMOGRAPHY),
    ((480, 640), (400, 600), [[0.93, -0.11, 31.0], [0.08, 1.04, -12.5], [1.2e-4, -6.0e-5, 1.0]]),
    ((200, 260), (300, 280), [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
    ((120, 160), (120, 160), [[0.5, 0.0, 200.0], [0.0, 0.5, 200.0], [0.0, 0.0, 1.0]]),       # no overlap at all
    ((480, 640), (480, 640), [[1.0, 0.0, 7.03125], [0.0, 1.0, -3.515625], [0.0, 0.0, 1.0]]),  # every coordinate ON a 1/32-px tie
    ((1080, 1920), (1080, 1920), [[0.98, 0.03, 11.0], [-0.02, 1.01, 5.0], [2.0e-5, -1.0e-5, 1.0]]),
]


def _probe_points(h, w, rng, n):
    """(x, y, radius, score) rows: on and around the mask frame, on half-integers (rounding ties), at row/column 0 (index -1
    wraps), and at arbitrary positions with multi-scale radii."""
    edge = np.array([0.0, 0.4, 0.5, 1.5, 13.5, 14.5, 15.0, 15.5, 16.0, 16.5])
    xs = np.concatenate([edge, w - 1 - edge, rng.integers(0, w, n // 4) + 0.5, rng.uniform(0, w - 1, n)])
    ys = np.concatenate([edge, h - 1 - edge, rng.integers(0, h, n // 4) + 0.5, rng.uniform(0, h - 1, n)])
    k = min(len(xs), len(ys))
    xs, ys = rng.permutation(xs[:k]), rng.permutation(ys[:k])
    xs, ys = np.clip(xs, 0, w - 1), np.clip(ys, 0, h - 1)
    rad = rng.choice([1.0, 1.4142135623730951, 2.0, 0.7071067811865476, 2.8284271247461903], k)
    return np.stack([xs, ys, rad, rng.uniform(0, 1, k)], axis=1)


def _composition(src, dst, hm, shape_src, shape_dst):
    """train_utils.py:344-379 with today's one-pair functions -> (kept src rows, warped kept dst rows, result or None)."""
    ms, md = geometry_tools.create_common_region_masks(hm, shape_src, shape_dst)
    idx_s = R.check_common_points(src[:, [1, 0, 2, 3]], ms)
    idx_d = R.check_common_points(dst[:, [1, 0, 2, 3]], md)
    ks = src[idx_s] if idx_s.size else np.zeros((0, 4))
    kd = dst[idx_d] if idx_d.size else np.zeros((0, 4))
    wd = geometry_tools.apply_homography_to_points(kd, hm) if len(kd) else np.zeros((0, 4))
    res = R.compute_repeatability(ks, wd) if len(ks) and len(kd) else None
    return ks, wd, res


def test_filter_and_warp_equal_the_composition():
    rng = np.random.default_rng(7)
    srcs, dsts, hs, shapes = [], [], [], []
    for rep in range(2):
        for shape_src, shape_dst, hm in MASK_CASES:
            srcs.append(_probe_points(*shape_src, rng, 300 + 200 * rep))
            dsts.append(_probe_points(*shape_dst, rng, 250 + 250 * rep))
            hs.append(np.asarray(hm, dtype=np.float64))
            shapes.append(shape_src + shape_dst)
    src, ns = _pack(srcs, max(map(len, srcs)), rng)
    dst, nd = _pack(dsts, max(map(len, dsts)), rng)
    h_dev = torch.from_numpy(np.stack(hs)).to(DEV)
    sh_dev = torch.tensor(shapes, dtype=torch.int32, device=DEV)
    cp = evaluate.common_points_batch(src, ns, dst, nd, h_dev, sh_dev)
    ev = _host(evaluate.evaluate_pairs(src, ns, dst, nd, h_dev, sh_dev))
    cs, cd, kept, valid = (t.cpu().numpy() for t in cp)
    assert np.array_equal(kept, ev["kept"]) and np.array_equal(valid, ev["valid"])
    n_valid = 0
    for p in range(len(srcs)):
        ks, wd, res = _composition(srcs[p], dsts[p], hs[p], shapes[p][:2], shapes[p][2:])
        assert kept[p, 0] == len(ks) and kept[p, 1] == len(wd), (p, kept[p], len(ks), len(wd))
        assert np.array_equal(cs[p, :len(ks)].view(np.uint64), ks.view(np.uint64)), p
        assert np.array_equal(cd[p, :len(wd)].view(np.uint64), wd.view(np.uint64)), p
        assert not cs[p, len(ks):].any() and not cd[p, len(wd):].any()
        assert bool(valid[p]) == (res is not None), p
        if res is not None:
            _same_as_single(ev, p, res)
            n_valid += 1
    assert 0 < n_valid < len(srcs)                               # the no-overlap pairs are invalid


# ---- the driver ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    out = {}
    for prec in ("fp32", "fp16"):
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(synth.synthetic_state_dict(cases.WEIGHT_SEED))
        m.precision = prec
        out[prec] = m.eval().to(DEV)
    return out


class _Loader:
    """3 sequences x 5 pairs, two image shapes: translated and cropped copies of a synthetic image, known homographies;
    sequence 2 holds a pair that does not overlap at all."""

    def __init__(self):
        self.sequences = ["a", "b", "c"]
        self._data = []
        for s, (h, w) in enumerate([(240, 320), (200, 264), (240, 320)]):
            g = synth.synthetic_gray_u8(h + 40, w + 40, 20 + s)
            src = synth.gray_to_rgb_norm(g[20:20 + h, 20:20 + w])
            dsts, hs = [], []
            for k in range(5):
                dy, dx = (3 * k - 6, 4 - 2 * k) if s != 2 or k < 2 else (k, -k)
                hh, ww = (h, w) if s != 2 or k < 2 else (200, 264)          # sequence 2: destinations of another shape
                dsts.append(synth.gray_to_rgb_norm(g[20 + dy:20 + dy + hh, 20 + dx:20 + dx + ww]))
                hs.append(np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]]))
            if s == 2:
                hs[4] = np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # no common region
            self._data.append(dict(sequence_name=self.sequences[s], im_src_RGB_norm=src, images_dst_RGB_norm=dsts,
                                   h_dst_2_src=hs))

    def get_sequence_data(self, i):
        return self._data[i]


def _reference_loop(loader, model, nms_size=15, num_points=25, border_size=15, multi_scale=False):
    """The reference's loop body (train_utils.py:331-379) with today's one-pair functions."""
    rep_s, rep_m, err_s, err_m, poss = [], [], [], [], []
    for i in range(len(loader.sequences)):
        sd = loader.get_sequence_data(i)
        src_im, dst_ims, hs = sd["im_src_RGB_norm"], sd["images_dst_RGB_norm"], sd["h_dst_2_src"]
        for k in range(len(dst_ims)):
            if multi_scale:
                pts_src = MS.extract_multiscale_detections(src_im, model, DEV, nms_size=nms_size, num_points=num_points,
                                                           border_size=border_size)
                pts_dst = MS.extract_multiscale_detections(dst_ims[k], model, DEV, nms_size=nms_size, num_points=num_points,
                                                           border_size=border_size)
            else:
                pts_src, _ = pipeline.extract_detections(src_im, model, DEV, nms_size=nms_size, num_points=num_points,
                                                         border_size=border_size)
                pts_dst, _ = pipeline.extract_detections(dst_ims[k], model, DEV, nms_size=nms_size, num_points=num_points,
                                                         border_size=border_size)
            mask_src, mask_dst = geometry_tools.create_common_region_masks(hs[k], src_im.shape, dst_ims[k].shape)
            pts_src = np.asarray(list(map(lambda x: [x[1], x[0], x[2], x[3]], pts_src)))
            pts_dst = np.asarray(list(map(lambda x: [x[1], x[0], x[2], x[3]], pts_dst)))
            idx_src = R.check_common_points(pts_src, mask_src)
            if idx_src.size == 0:
                continue
            pts_src = pts_src[idx_src]
            idx_dst = R.check_common_points(pts_dst, mask_dst)
            if idx_dst.size == 0:
                continue
            pts_dst = pts_dst[idx_dst]
            pts_src = np.asarray(list(map(lambda x: [x[1], x[0], x[2], x[3]], pts_src)))
            pts_dst = np.asarray(list(map(lambda x: [x[1], x[0], x[2], x[3]], pts_dst)))
            pts_dst_to_src = geometry_tools.apply_homography_to_points(pts_dst, hs[k])
            r = R.compute_repeatability(pts_src, pts_dst_to_src)
            rep_s.append(r["rep_single_scale"])
            rep_m.append(r["rep_multi_scale"])
            err_s.append(r["error_overlap_single_scale"])
            err_m.append(r["error_overlap_multi_scale"])
            poss.append(r["possible_matches"])
    return (np.asarray(rep_s).mean(), np.asarray(rep_m).mean(), np.asarray(err_s).mean(), np.asarray(err_m).mean(),
            np.asarray(poss).mean()), len(rep_s)


def _equal(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert np.array_equal(np.float64(x), np.float64(y)), (a, b)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_driver_equals_reference_loop(models, precision):
    m = models[precision]
    loader = _Loader()
    with torch.inference_mode():
        ref, n_pairs = _reference_loop(loader, m, num_points=60)
        got = train_utils.check_val_hsequences_repeatability(loader, m, DEV, None, 0, num_points=60)
        again = train_utils.check_val_hsequences_repeatability(loader, m, DEV, None, 0, num_points=60, chunk_sequences=1,
                                                               batch_size=2)
    assert m.effective_precision == precision
    assert n_pairs == 14                                         # the non-overlapping pair is skipped
    assert 0.0 < float(ref[0]) <= 100.0
    _equal(got, ref)
    _equal(again, ref)


def test_driver_multi_scale_equals_reference_loop(models):
    m = models["fp16"]
    loader = _Loader()
    with torch.inference_mode():
        ref, n_pairs = _reference_loop(loader, m, num_points=300, multi_scale=True)
        got = train_utils.check_val_hsequences_repeatability(loader, m, DEV, None, 0, num_points=300, multi_scale=True)
    assert n_pairs == 14
    _equal(got, ref)


def test_driver_rejects_tb_log(models):
    with pytest.raises(NotImplementedError):
        train_utils.check_val_hsequences_repeatability(_Loader(), models["fp32"], DEV, object(), 0)


def test_driver_sizes_the_candidate_buffer_from_the_totals(models, monkeypatch):
    m = models["fp32"]
    loader = _Loader()
    with torch.inference_mode():
        big = train_utils.check_val_hsequences_repeatability(loader, m, DEV, None, 0, num_points=60)
        monkeypatch.setattr(R, "MAX_EDGES", 8)                   # the default buffer: far too small for these pairs
        small = train_utils.check_val_hsequences_repeatability(loader, m, DEV, None, 0, num_points=60)
    _equal(small, big)


# ---- overflow and stream order ------------------------------------------------------------------------------------------
def test_overflow_reports_exactly_the_pairs_that_do_not_fit():
    rng = np.random.default_rng(1)
    crowd = np.concatenate([rng.uniform(50, 60, (300, 2)), np.full((300, 1), 20.0), rng.uniform(0, 1, (300, 1))], axis=1)
    pairs = []
    for k in range(12):
        pairs.append((crowd, crowd + 0.25) if k % 3 == 1 else cases.repeat_inputs(dict(ns=200, nd=180, seed=50 + k,
                                                                                          planted=120)))
    src, ns = _pack([a for a, _ in pairs], 300, rng)
    dst, nd = _pack([b for _, b in pairs], 300, rng)
    big = _host(R.compute_repeatability_batch(src, ns, dst, nd))
    cand = np.stack([big["candidates_single_scale"], big["candidates_multi_scale"]], axis=1).astype(np.int64)
    assert (cand[1::3] > 10000).all()
    max_edges = int(cand[:5, 0].sum() + 5)                       # pairs 0..4 of the single scale fit, pair 5 does not
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    torch.cuda._sleep(int(1.5e9))
    t0 = time.perf_counter()
    res = R.compute_repeatability_batch(src, ns, dst, nd, max_edges=max_edges)
    dt = time.perf_counter() - t0
    done.record()
    busy = not done.query()
    got = _host(res)
    assert busy and dt < 0.1, (busy, dt)                         # nothing waited for the device
    for which, name in ((0, "single_scale"), (1, "multi_scale")):
        end = np.cumsum(cand[:, which])
        over = end > max_edges
        assert over.any() and not over.all()
        assert np.array_equal(got[f"candidates_{name}"], big[f"candidates_{name}"])
        assert np.array_equal(got[f"num_points_{name}"] == -1, over), name
        assert np.isnan(got[f"rep_{name}"][over]).all()
        fit = ~over
        for k in (f"num_points_{name}", f"rep_{name}", f"error_overlap_{name}"):
            assert np.array_equal(got[k][fit], big[k][fit]), k
    for k in ("possible_matches", "total_num_points"):
        assert np.array_equal(got[k], big[k])


def _nan_equal(a, b):
    if a.is_floating_point():
        a, b = a.nan_to_num(-7.0), b.nan_to_num(-7.0)
    return torch.equal(a, b)


def test_evaluate_pairs_replays_in_a_graph():
    p, n = 16, 400

    def make(seed):
        r = np.random.default_rng(seed)
        srcs, dsts, hs = [], [], []
        for _ in range(p):
            s = _probe_points(480, 640, r, n - 140)
            hm = np.array([[1.0 + r.normal(0, 0.02), r.normal(0, 0.02), r.normal(0, 8)],
                           [r.normal(0, 0.02), 1.0 + r.normal(0, 0.02), r.normal(0, 8)],
                           [r.normal(0, 2e-5), r.normal(0, 2e-5), 1.0]])
            d = geometry_tools.apply_homography_to_points(s, np.linalg.inv(hm))
            d[:, :2] += r.normal(0, 1.0, (len(d), 2))
            d[:, :2] = np.clip(d[:, :2], 0, [639, 479])
            srcs.append(s[:int(r.integers(0, n))])
            dsts.append(d[:int(r.integers(1, n))])
            hs.append(hm)
        src, ns = _pack(srcs, n, r)
        dst, nd = _pack(dsts, n, r)
        return (src, ns, dst, nd, torch.from_numpy(np.stack(hs)).to(DEV),
                torch.tensor([[480, 640, 480, 640]] * p, dtype=torch.int32, device=DEV))

    static = make(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            evaluate.evaluate_pairs(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = evaluate.evaluate_pairs(*static)
    for seed in (10, 20):
        new = make(seed)
        for a, b in zip(static, new):
            a.copy_(b)
        graph.replay()
        got = {k: v.clone() for k, v in out._asdict().items()}
        ref = evaluate.evaluate_pairs(*new)
        torch.cuda.synchronize()
        assert int(ref.valid.sum()) > 0
        for k, v in ref._asdict().items():
            assert _nan_equal(got[k], v), k
