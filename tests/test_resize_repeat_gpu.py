"""The resize protocol on the GPU (balf_resize_repeatability_batch / balf_resize_crop_u8 in include/balf_hip.h; their Python
layers) against tests/golden/resize_repeat.npz -- recorded from the reference's own functions by
tests/golden/make_resize_golden.py --, against the NumPy restatements of tests/resize_repeat_common.py and against the loop over
this package's one-pair functions.  Only the fixture is read here, never the reference tree."""
import types

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.benchmark_test import evaluate, repeatability_tools as RT
from balf_amd.datasets import dataset_utils
from balf_amd.model import get_model
from balf_amd.pipeline import detect_batch_u8
from balf_amd.utils import synth
from tests import resize_repeat_common as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return R.fixture()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- 1. the golden cases -------------------------------------------------------------------------------------------------
def test_golden_cases_one_pair(g):
    """Counts equal, repeatability bit-equal (one float64 expression of four integers), localization_err within 1e-9
    absolute.  Derived, not measured: coordinates are below 2^12, a warp is about ten float64 operations (|error| <= ~4e-12
    per coordinate; BLAS in the reference may fuse differently), the distance inherits about twice that, a mean of <= 2000
    terms <= 5 adds <= 1.2e-12 for the order of summation: < 2e-11 in all, 1e-9 leaves a factor 50."""
    for n in R.case_names(g):
        src, dst, h, ss, sd, k, thr = R.case_inputs(g, n)
        keep_s, keep_d = src.copy(), dst.copy()
        r = RT.compute_resize_repeatability(src, dst, h, ss, sd, keep_k_points=k, distance_thresh=thr)
        assert list(r) == list(R.KEYS)
        assert np.array_equal(src, keep_s) and np.array_equal(dst, keep_d), n          # the inputs are NOT overwritten
        print(n, {key: float(r[key]) for key in R.KEYS}, "want", {key: float(g[f"{n}.{key}"]) for key in R.KEYS})
        for key in R.KEYS[2:]:
            assert int(r[key]) == int(g[f"{n}.{key}"]), (n, key)
        assert np.float64(r["repeatability"]) == np.float64(g[f"{n}.repeatability"]), n
        assert abs(float(r["localization_err"]) - float(g[f"{n}.localization_err"])) < 1e-9, n


def test_value_types_are_the_references(g):
    src, dst, h, ss, sd, k, thr = R.case_inputs(g, "both_above_k")
    r = RT.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    assert isinstance(r["repeatability"], np.float64) and isinstance(r["localization_err"], np.float64)
    assert type(r["common_src_num"]) is int and isinstance(r["rep_src_num"], np.int64)
    src, dst, h, ss, sd, k, thr = R.case_inputs(g, "both_empty")
    r = RT.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    assert r["repeatability"] == 0. and type(r["repeatability"]) is float
    assert r["localization_err"] == -1 and type(r["localization_err"]) is int and type(r["rep_src_num"]) is int


def test_source_array_can_be_reused_for_a_second_destination(g):
    """The reference writes the warped coordinates into the caller's `keypoints`; here the same array scores a second
    destination as a fresh copy does."""
    src, dst, h, ss, sd, k, thr = R.case_inputs(g, "neither_above_k")
    first = RT.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    again = RT.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    assert all(np.array_equal(first[key], again[key]) for key in R.KEYS)


def test_tie_at_the_cut_follows_the_documented_rule():
    """Many rows of equal prob at the cut (the reference's choice there is arbitrary): against the restatement only."""
    src, dst, h, ss, sd, k, thr = R.tie_case()
    want, _, _ = R.resize_repeatability_np(src, dst, h, ss, sd, k, thr)
    got = RT.compute_resize_repeatability(src, dst, h, ss, sd, k, thr)
    assert want["common_src_num"] == k and want["common_dst_num"] == k
    for key in R.KEYS[2:]:
        assert int(got[key]) == int(want[key]), key
    assert np.float64(got["repeatability"]) == np.float64(want["repeatability"])
    assert abs(float(got["localization_err"]) - float(want["localization_err"])) < 1e-9
    # a different choice among the ties would give different counts: dropping the tie rule (the HIGHER index) changes them
    rev_s, rev_d = src[::-1].copy(), dst[::-1].copy()
    other, _, _ = R.resize_repeatability_np(rev_s, rev_d, h, ss, sd, k, thr)
    assert (other["rep_src_num"], other["rep_dst_num"]) != (want["rep_src_num"], want["rep_dst_num"])


# ---- 2. the batch equals the one-pair call ---------------------------------------------------------------------------------
def _batch_inputs(g, p, rng):
    """P pairs from the fixture's cases in random order plus random prefixes: ragged counts, rows past a count NaN."""
    names = [n for n in R.case_names(g) if tuple(g[f"{n}.shape_dst"]) == (240, 320)] + ["unequal_shapes"]
    pairs = []
    for i in range(p):
        src, dst, h, ss, sd, _, _ = R.case_inputs(g, names[int(rng.integers(len(names)))] if i >= len(names) else names[i])
        if i >= len(names):
            src, dst = src[:int(rng.integers(0, len(src) + 1))], dst[:int(rng.integers(0, len(dst) + 1))]
        pairs.append((src, dst, h, ss + sd))
    ns_max, nd_max = max(len(q[0]) for q in pairs), max(len(q[1]) for q in pairs)
    src = np.full((p, ns_max, 3), np.nan)
    dst = np.full((p, nd_max, 3), np.nan)
    for i, q in enumerate(pairs):
        src[i, :len(q[0])], dst[i, :len(q[1])] = q[0], q[1]
    ns, nd = np.asarray([len(q[0]) for q in pairs], np.int32), np.asarray([len(q[1]) for q in pairs], np.int32)
    return src, ns, dst, nd, np.stack([q[2] for q in pairs]), np.asarray([q[3] for q in pairs], np.int32)


def _run_batch(src, ns, dst, nd, h, shapes, k, thr, **kw):
    r = RT.compute_resize_repeatability_batch(_dev(src), _dev(ns), _dev(dst), _dev(nd), h, shapes, k, thr, **kw)
    return {f: getattr(r, f).cpu().numpy() for f in r._fields}


@pytest.mark.parametrize("p", [1, 7, 64])
@pytest.mark.parametrize("k,thr", [(1000, 5), (300, 3)])
def test_batch_equals_the_one_pair_call(g, p, k, thr):
    rng = np.random.default_rng([3, p, k])
    src, ns, dst, nd, h, shapes = _batch_inputs(g, p, rng)
    ws = ops._workspace("resize_repeat", torch.device(DEV), 1 << 24)
    ws.fill_(0xFF)                                                   # garbage in the workspace must not matter
    src_t, dst_t = _dev(src), _dev(dst)
    r = RT.compute_resize_repeatability_batch(src_t, _dev(ns), dst_t, _dev(nd), h, shapes, k, thr)
    got = {f: getattr(r, f).cpu().numpy() for f in r._fields}
    assert np.array_equal(src_t.cpu().numpy(), src, equal_nan=True) and np.array_equal(dst_t.cpu().numpy(), dst, equal_nan=True)
    for i in range(p):
        one = RT.compute_resize_repeatability(src[i, :ns[i]], dst[i, :nd[i]], h[i], shapes[i, :2], shapes[i, 2:], k, thr)
        for f in R.KEYS:
            assert np.array_equal(np.asarray(got[f][i], np.float64), np.asarray(one[f], np.float64)), (i, f, got[f][i], one[f])
    perm = rng.permutation(p)
    again = _run_batch(src[perm], ns[perm], dst[perm], nd[perm], h[perm], shapes[perm], k, thr)
    for f in R.KEYS:
        assert np.array_equal(again[f], got[f][perm]), f
    assert p < 64 or ((got["common_src_num"] == 0).any() and (got["rep_src_num"] > 0).any())
    # the detector's row layout through the order flag: (x, y, radius, score) rows give the same results
    xyrs_s = np.stack([src[..., 1], src[..., 0], np.ones_like(src[..., 0]), src[..., 2]], axis=-1)
    xyrs_d = np.stack([dst[..., 1], dst[..., 0], np.ones_like(dst[..., 0]), dst[..., 2]], axis=-1)
    flag = _run_batch(xyrs_s, ns, xyrs_d, nd, h, shapes, k, thr, order="xyrs")
    for f in R.KEYS:
        assert np.array_equal(flag[f], got[f]), f


def test_c_abi_stays_inside_its_buffers(g):
    """Straight through ctypes with caller-owned buffers between guard bands: a 0xFF workspace of exactly the size asked for,
    outputs pre-filled with garbage, rows past every count NaN, twice."""
    from tests.test_guard_gpu import Guarded
    l = _lib.lib()
    p, k, thr = 7, 300, 3.0
    src, ns, dst, nd, h, shapes = _batch_inputs(g, p, np.random.default_rng(17))
    want = _run_batch(src, ns, dst, nd, h, shapes, k, thr)
    ns_max, nd_max = src.shape[1], dst.shape[1]
    src_t, dst_t, ns_t, nd_t = _dev(src), _dev(dst), _dev(ns), _dev(nd)
    h_t, hi_t, sh_t = _dev(h), _dev(np.linalg.inv(h)), _dev(shapes)
    nbytes = l.balf_resize_repeatability_batch_workspace_bytes(p, ns_max, nd_max, k)
    assert nbytes > 0
    ws = Guarded(nbytes, fill=0xFF)
    rep, cnt = Guarded(p * 16, fill=0x7B), Guarded(p * 16, fill=0x7B)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream

    def call(ws_bytes):
        return l.balf_resize_repeatability_batch(src_t.data_ptr(), ns_t.data_ptr(), ns_max, 3, dst_t.data_ptr(), nd_t.data_ptr(),
                                                 nd_max, 3, 1, 0, p, h_t.data_ptr(), hi_t.data_ptr(), sh_t.data_ptr(), k, thr,
                                                 rep.ptr, cnt.ptr, ws.ptr, ws_bytes, stream)

    for _ in range(2):                                               # the second call finds the first one's workspace
        assert call(nbytes) == 0
        torch.cuda.synchronize()
        assert ws.intact() and rep.intact() and cnt.intact()
        got_rep, got_cnt = rep.view(torch.float64, (p, 2)).cpu().numpy(), cnt.view(torch.int32, (p, 4)).cpu().numpy()
        assert np.array_equal(got_rep[:, 0], want["repeatability"]) and np.array_equal(got_rep[:, 1], want["localization_err"])
        assert np.array_equal(got_cnt, np.stack([want[f] for f in R.KEYS[2:]], axis=1))
    assert call(nbytes - 1) == -3                                    # BALF_ERR_WORKSPACE
    assert np.array_equal(src_t.cpu().numpy(), src, equal_nan=True) and np.array_equal(dst_t.cpu().numpy(), dst, equal_nan=True)


# ---- 3. the resize -------------------------------------------------------------------------------------------------------
# (the last two: one-pixel-thin sources, a single tap on one axis)
RESIZE_SIZES = ((480, 640), (300, 700), (700, 300), (100, 120), (333, 517), (125, 175), (241, 320), (240, 325), (50, 25), (1, 37),
                (41, 1))


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("target", [(240, 320), (5, 2), (67, 130), (1, 65)])
def test_resize_equals_the_integer_restatement(color, target):
    """Sizes that crop in x, in y, that need upscaling, odd sizes (125 x 175 at scale 0.02 -> 2.5 and 3.5, 50 x 25 at 0.1 -> 2.5:
    np.round goes to even) and odd differences; images of different sizes in ONE call; integer arithmetic: array_equal.
    Targets of whole 64 x 4 tiles, of one partial tile, of whole and partial tiles on both axes (67 x 130), of a single row."""
    rng = np.random.default_rng(8)
    images = []
    for i, (h, w) in enumerate(RESIZE_SIZES):
        im = synth.synthetic_gray_u8(h, w, 60 + i) if i % 2 == 0 else rng.integers(0, 256, (h, w), dtype=np.uint8)
        images.append(np.stack([im, 255 - im, im // 2 + 7], axis=2) if color else im)
    out = dataset_utils.ratio_preserving_resize_batch(images, target).cpu().numpy()
    assert out.shape == (len(images),) + target + ((3,) if color else ()) and out.dtype == np.uint8
    for i, im in enumerate(images):
        want = R.ratio_preserving_resize_np(im, target)
        assert np.array_equal(out[i], want), (i, im.shape, np.abs(out[i].astype(int) - want.astype(int)).max())
        one = dataset_utils.ratio_preserving_resize(im, target)
        assert isinstance(one, np.ndarray) and np.array_equal(one, want), i
    assert out.any()


def test_resize_rejects_an_image_outside_the_buffer():
    """A size / offset pair that does not lie inside the packed buffer gives a zero image instead of a read out of bounds."""
    im = np.full((7, 9), 200, np.uint8)
    packed, off = _dev(im.reshape(-1)), _dev(np.asarray([0, 8], np.int64))
    sizes = _dev(np.asarray([[7, 9], [7, 9]], np.int32))
    out = ops.resize_crop_u8(packed, off, sizes, 1, 14, 18).cpu().numpy()
    assert np.array_equal(out[0], R.ratio_preserving_resize_np(im, (14, 18))) and out[0].all()
    assert not out[1].any()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    out = {}
    for prec in ("fp32", "fp16"):
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(synth.synthetic_state_dict(3))
        m.precision = prec
        out[prec] = m.eval().to(DEV)
    return out


def _one_pair_loop(loader, m, shape, top_k, thr, nms, border):
    """The protocol from the one-image / one-pair functions; 3-channel loader images are reversed to RGB by hand."""
    args = types.SimpleNamespace(resize_shape=list(shape))

    def rows_of(img):
        img = np.ascontiguousarray(img[:, :, ::-1]) if img.ndim == 3 else img
        small = dataset_utils.ratio_preserving_resize(img, shape)
        idx, score, count, _ = detect_batch_u8(m, torch.from_numpy(small).to(DEV)[None], border, nms, top_k)
        n = int(count[0])
        i = idx[0, :n].cpu().numpy().astype(np.int64)
        return np.stack([i // shape[1], i % shape[1], score[0, :n].cpu().numpy().astype(np.float64)], axis=1)

    out = {key: [] for key in R.KEYS}
    for s in range(len(loader.sequences)):
        d = loader.get_sequence_data(s)
        src_rows = rows_of(d['im_src_BGR'])
        for dst, h in zip(d['images_dst_BGR'], d['homographies']):
            hh = dataset_utils.adapt_homography_to_preprocessing(
                {'homography': h, 'shape': np.array(d['im_src_BGR'].shape[:2]), 'warped_shape': np.array(dst.shape[:2])}, args)
            r = RT.compute_resize_repeatability(src_rows, rows_of(dst), hh, shape, shape, keep_k_points=top_k, distance_thresh=thr)
            for key in R.KEYS:
                out[key].append(r[key])
    return out


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("color", [False, True])
def test_evaluate_resize_hsequences_equals_the_one_pair_loop(models, precision, color):
    m = models[precision]
    loader = R.SyntheticSequences(n_sequences=3, n_dst=2, color=color)
    with torch.inference_mode():
        got = evaluate.evaluate_resize_hsequences(loader, m, DEV, top_k_points=300, pixel_threshold=3)
        small = evaluate.evaluate_resize_hsequences(loader, m, DEV, top_k_points=300, pixel_threshold=3, chunk_sequences=2,
                                                    batch_size=2)
        want = _one_pair_loop(loader, m, (240, 320), 300, 3, 15, 15)
    assert m.effective_precision == precision
    assert got["sequences"] == loader.sequences and got["top_k"] == 300 and got["pixel_threshold"] == 3
    print(precision, color, {key: got[key] for key in R.KEYS})
    for key in R.KEYS:
        assert len(got[key]) == 6
        assert np.array_equal(np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)), (key, got[key], want[key])
        assert got[key] == small[key], key
    assert min(got["common_src_num"]) > 0 and min(got["common_dst_num"]) > 0 and max(got["repeatability"]) > 0.0
    if color:                                                        # the channel order matters: BGR taken as RGB differs
        class AsRgb:
            sequences = loader.sequences

            @staticmethod
            def get_sequence_data(i):
                d = dict(loader.get_sequence_data(i))
                d['im_src_BGR'] = np.ascontiguousarray(d['im_src_BGR'][:, :, ::-1])
                d['images_dst_BGR'] = [np.ascontiguousarray(x[:, :, ::-1]) for x in d['images_dst_BGR']]
                return d
        with torch.inference_mode():
            other = evaluate.evaluate_resize_hsequences(AsRgb, m, DEV, top_k_points=300, pixel_threshold=3)
        assert any(other[key] != got[key] for key in R.KEYS)


# ---- 5. stream order: capture and replay -----------------------------------------------------------------------------------
def test_core_captured_in_a_graph_replays_bit_identical(g):
    """Nothing inside synchronises or reads back: with h and inv(h) on the device the core is captured with torch.cuda.graph
    and the replays (other inputs copied into the captured buffers, then the first again) equal the eager calls bit for bit."""
    rng = np.random.default_rng(23)
    k, thr = 300, 5
    a_np = _batch_inputs(g, 7, rng)
    perm = rng.permutation(7)
    b_np = tuple(x[perm] for x in a_np)
    sets = []
    for src, ns, dst, nd, h, shapes in (a_np, b_np):
        sets.append([_dev(src), _dev(ns), _dev(dst), _dev(nd), _dev(h), _dev(np.linalg.inv(h)), _dev(shapes)])

    def core(t):
        return evaluate.evaluate_resize_pairs(t[0], t[1], t[2], t[3], t[4], t[6], k, thr, h_inv=t[5], order="rcp")

    eager = [[x.clone() for x in core(t)] for t in sets]
    torch.cuda.synchronize()
    buf = [x.clone() for x in sets[0]]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(side):                                    # warm-up on the capture stream: workspaces
        core(buf)
    torch.cuda.current_stream(torch.device(DEV)).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = core(buf)
    for which in (0, 1, 0):
        for b, x in zip(buf, sets[which]):
            b.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for got_t, want_t, f in zip(out, eager[which], out._fields):
            assert np.array_equal(got_t.cpu().numpy(), want_t.cpu().numpy()), (which, f)
