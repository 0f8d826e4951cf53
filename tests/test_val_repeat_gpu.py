"""check_val_repeatability on the GPU (balf_val_points in include/balf_hip.h; ops.val_points, evaluate.evaluate_val_pairs,
train_utils.check_val_repeatability) against tests/golden/val_repeat.npz -- recorded from the reference's own functions by
tests/golden/make_val_golden.py -- and against the loop over this package's one-pair functions, bit for bit.  Only the
fixture is read here, never the reference tree."""
import warnings as W

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.benchmark_test import evaluate, geometry_tools
from balf_amd.model import get_model
from balf_amd.utils import synth, train_utils
from tests import val_repeat_common as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = V.REP_KEYS + V.COUNT_KEYS


@pytest.fixture(scope="module")
def g():
    return V.fixture()


@pytest.fixture(scope="module")
def models(g):
    out = {}
    for prec in ("fp32", "fp16"):
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(synth.synthetic_state_dict(int(g["meta.weight_seed"])))
        m.precision = prec
        out[prec] = m.eval().to(DEV)
    return out


def _groups(g, names):
    """names grouped by (source shape, destination shape): one call of the batched entry per group."""
    out = {}
    for n in names:
        out.setdefault((g[f"{n}.prob_src"].shape, g[f"{n}.prob_dst"].shape), []).append(n)
    return list(out.values())


def _stack(g, names):
    return (torch.from_numpy(np.stack([g[f"{n}.prob_src"] for n in names])).to(DEV),
            torch.from_numpy(np.stack([g[f"{n}.prob_dst"] for n in names])).to(DEV),
            torch.from_numpy(np.stack([g[f"{n}.h_dst_2_src"] for n in names])).to(DEV))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. identical input: the recorded score maps through the new selection -------------------------------------------------
@pytest.mark.parametrize("leg", V.LEGS)
def test_selection_on_recorded_maps_is_the_references(g, leg):
    """Rows, their order and the counts are bit-identical to get_point_coordinates' on the reference's masked NMS maps, the
    fallback pairs included ("thin": fewer than K positive values; "zero": none, the first K raster pixels).  The warped
    destination rows: position and radius within 1e-12 of apply_homography_to_points (the reference goes through
    np.linalg.inv / eig there, the kernel through the closed form; the bar of test_repeat_batch_gpu.py), score bit-identical."""
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    seen = set()
    for names in _groups(g, V.map_names(g)):
        ps, pd, h = _stack(g, names)
        src, dst, count = ops.val_points(ps, pd, h, nms, k, leg)
        src, dst, count = src.cpu().numpy(), dst.cpu().numpy(), count.cpu().numpy()
        for p, n in enumerate(names):
            want_s, want_d, want_w = g[f"{n}.{leg}.src"], g[f"{n}.{leg}.dst"], g[f"{n}.{leg}.dst_to_src"]
            assert tuple(count[p]) == (len(want_s), len(want_d)), (n, leg, count[p])
            assert np.array_equal(_bits(src[p, :len(want_s)]), _bits(want_s)), (n, leg)
            assert not src[p, len(want_s):].any() and not dst[p, len(want_d):].any(), (n, leg)
            got_w = dst[p, :len(want_d)]
            assert np.array_equal(_bits(got_w[:, 3]), _bits(want_w[:, 3])), (n, leg)
            assert np.abs(got_w[:, :3] - want_w[:, :3]).max() < 1e-12, (n, leg)
            # the destination rows BEFORE the warp, bit for bit: the recorded rows warped by this package's own one-point entry
            # (the same arithmetic) are the kernel's rows
            assert np.array_equal(_bits(geometry_tools.apply_homography_to_points(want_d, g[f"{n}.h_dst_2_src"])), _bits(got_w)), (n, leg)
            seen.add(n)
    assert {"thin", "zero", "shapes", "black", "mild"} <= seen


# ---- 2. the batched core equals the loop over the one-pair functions -------------------------------------------------------
def _synthetic_maps(rng, h, w, kind):
    if kind == "zero":
        return np.zeros((h, w), np.float32)
    if kind == "flat":                                              # a plateau: window NMS keeps every pixel, all ties
        return np.full((h, w), 0.25, np.float32)
    if kind == "ties":                                              # few distinct values: ties at the K-th value
        return (rng.integers(0, 6, (h, w)) / 8.0).astype(np.float32)
    if kind == "sparse":
        m = np.zeros((h, w), np.float32)
        at = rng.choice(h * w, 40, replace=False)
        m.ravel()[at] = rng.uniform(0.02, 1.0, 40).astype(np.float32)
        return m
    return rng.random((h, w), dtype=np.float32)


@pytest.mark.parametrize("leg", V.LEGS)
def test_evaluate_val_pairs_equals_the_one_pair_loop(g, leg):
    """P pairs in one batch (the fixture's maps plus synthetic ones: all-zero, a plateau, tie-heavy, sparse, random; thin and
    empty common regions) against create_common_region_masks / apply_nms or greedy_nms + scatter / get_point_coordinates /
    apply_homography_to_points / compute_repeatability per pair: every field equal bit for bit (NaN-aware)."""
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    rng = np.random.default_rng(11)
    names = [n for n in V.map_names(g) if g[f"{n}.prob_dst"].shape == (128, 128)]
    maps_s = [g[f"{n}.prob_src"] for n in names]
    maps_d = [g[f"{n}.prob_dst"] for n in names]
    hs = [g[f"{n}.h_dst_2_src"] for n in names]
    shift = np.array([[1.0, 0.0, 90.0], [0.0, 1.0, 1.0], [0.0, 0.0, 1.0]])          # a strip 8 pixels wide
    gone = np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])         # no common region: both fallbacks
    for kind, h in (("zero", hs[0]), ("flat", hs[0]), ("flat", shift), ("ties", hs[1]), ("sparse", hs[0]), ("random", shift),
                    ("random", gone), ("ties", gone)):
        maps_s.append(_synthetic_maps(rng, 128, 128, kind))
        maps_d.append(_synthetic_maps(rng, 128, 128, kind))
        hs.append(h)
    ps = torch.from_numpy(np.stack(maps_s)).to(DEV)
    pd = torch.from_numpy(np.stack(maps_d)).to(DEV)
    hh = torch.from_numpy(np.stack(hs)).to(DEV)
    ws = ops._workspace("val_points", torch.device(DEV), 1 << 26)
    ws.fill_(0xFF)                                                   # garbage in the workspace must not matter
    r = evaluate.evaluate_val_pairs(ps, pd, hh, nms, k, leg=leg)
    got = {f: getattr(r, f).cpu().numpy() for f in r._fields}
    src, dst, count = (t.cpu().numpy() for t in ops.val_points(ps, pd, hh, nms, k, leg))
    assert np.array_equal(got["kept"], count) and got["valid"].all()
    short = 0
    for p in range(len(hs)):
        want_s, want_w, want = V.gpu_loop_pair(maps_s[p], maps_d[p], hs[p], nms, k, leg)
        assert tuple(count[p]) == (len(want_s), len(want_w)), (p, count[p])
        assert np.array_equal(_bits(src[p, :count[p, 0]]), _bits(want_s)), p
        assert np.array_equal(_bits(dst[p, :count[p, 1]]), _bits(want_w)), p
        assert not src[p, count[p, 0]:].any() and not dst[p, count[p, 1]:].any(), p
        for f in FIELDS:
            a, b = np.asarray(got[f][p]), np.asarray(want[f], dtype=got[f].dtype)
            assert np.array_equal(a, b, equal_nan=True), (p, f, a, b)
        short += count[p, 0] < k
    assert short >= 2


@pytest.mark.parametrize("leg", V.LEGS)
def test_c_abi_stays_inside_its_buffers(g, leg):
    """Straight through ctypes with caller-owned buffers between guard bands: a 0xFF workspace of exactly the size asked for,
    outputs pre-filled with garbage (rows past every count come out 0), two different shapes."""
    from tests.test_guard_gpu import Guarded
    l = _lib.lib()
    code = ops.VAL_LEGS[leg]
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    ps, pd, h = _stack(g, ["shapes", "shapes", "shapes"])
    p, (hs, ws_), (hd, wd) = 3, ps.shape[1:], pd.shape[1:]
    want = [t.cpu().numpy() for t in ops.val_points(ps, pd, h, nms, k, leg)]
    nbytes = l.balf_val_points_workspace_bytes(p, hs, ws_, hd, wd, code, nms, k)
    assert nbytes > 0
    ws = Guarded(nbytes, fill=0xFF)
    src, dst, cnt = Guarded(p * k * 32, fill=0x7B), Guarded(p * k * 32, fill=0x7B), Guarded(p * 8, fill=0x7B)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for _ in range(2):                                               # the second call finds the first one's workspace
        rc = l.balf_val_points(ps.data_ptr(), hs, ws_, pd.data_ptr(), hd, wd, p, h.data_ptr(), code, 0.015, nms, k, src.ptr,
                               dst.ptr, cnt.ptr, ws.ptr, nbytes, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert ws.intact() and src.intact() and dst.intact() and cnt.intact()
        assert np.array_equal(src.view(torch.float64, (p, k, 4)).cpu().numpy(), want[0])
        assert np.array_equal(dst.view(torch.float64, (p, k, 4)).cpu().numpy(), want[1])
        assert np.array_equal(cnt.view(torch.int32, (p, 2)).cpu().numpy(), want[2])
    assert l.balf_val_points(ps.data_ptr(), hs, ws_, pd.data_ptr(), hd, wd, p, h.data_ptr(), code, 0.015, nms, k, src.ptr, dst.ptr,
                             cnt.ptr, ws.ptr, nbytes - 1, stream) == -3                     # BALF_ERR_WORKSPACE
    assert l.balf_val_points(ps.data_ptr(), hs, ws_, pd.data_ptr(), hd, wd, p, h.data_ptr(), code, 0.015, nms, hs * ws_ + 1,
                             src.ptr, dst.ptr, cnt.ptr, ws.ptr, nbytes, stream) < 0
    with pytest.raises(IndexError):
        ops.val_points(ps, pd, h, nms, hs * ws_ + 1, leg)


# ---- 3. end to end against the reference's ten means -----------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_check_val_repeatability_against_the_reference(g, models, precision):
    """The forward here is within 6e-6 of the reference's; the fixture's pairs were recorded under the condition that
    perturbing the reference's score maps by +-2e-5 does not change any selected point set (make_val_golden.py), so the
    counts are equal and the ten means agree to 1e-9.  No pair is skipped."""
    m = models[precision]
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    loader = V.fixture_loader(g)
    with torch.inference_mode():
        got = train_utils.check_val_repeatability(loader, m, DEV, None, 0, nms_size=nms, num_points=k)
        again = train_utils.check_val_repeatability(loader, m, DEV, None, 0, nms_size=nms, num_points=k, chunk_pairs=2,
                                                    batch_size=1)
        # per pair: the selected counts of both legs are the reference's
        for names in _groups(g, [str(n) for n in g["meta.names"]]):
            xs = torch.stack([V.to_input(g[f"{n}.image_src"]) for n in names]).to(DEV)
            xd = torch.stack([V.to_input(g[f"{n}.image_dst"]) for n in names]).to(DEV)
            ps, pd = m(xs, want_logits=False)["prob"], m(xd, want_logits=False)["prob"]
            h = torch.from_numpy(np.stack([g[f"{n}.h_dst_2_src"] for n in names])).to(DEV)
            for leg in V.LEGS:
                src, _, count = ops.val_points(ps, pd, h, nms, k, leg)
                src, count = src.cpu().numpy(), count.cpu().numpy()
                for p, n in enumerate(names):
                    assert tuple(count[p]) == (len(g[f"{n}.{leg}.src"]), len(g[f"{n}.{leg}.dst"])), (n, leg)
                    assert np.array_equal(src[p, :count[p, 0], :2], g[f"{n}.{leg}.src"][:, :2]), (n, leg)
                    assert np.abs(ps[p].cpu().numpy() - g[f"{n}.prob_src"]).max() < 2e-5, n
    assert m.effective_precision == precision
    assert len(got) == len(again) == 10
    print("ten means", precision, [float(v) for v in got])
    for i in range(10):
        assert abs(float(got[i]) - float(g["loader.ten"][i])) < 1e-9, (i, got, g["loader.ten"])
        assert np.array_equal(np.float64(got[i]), np.float64(again[i])), i


# ---- 4. the two quirks ------------------------------------------------------------------------------------------------------
def test_only_element_zero_counts_and_nms_values_are_the_last_pairs(g, models):
    m = models["fp32"]
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    loader = V.fixture_loader(g)
    assert max(len(b[0]) for b in loader) > 1
    alone = [tuple(t[:1] for t in b) for b in loader]                        # every batch cut down to its element 0
    other = [tuple(torch.cat([t[:1], torch.flip(t[1:], dims=(-1,)) * 0.5]) for t in b) for b in loader]   # elements 1.. changed
    with torch.inference_mode():
        full = train_utils.check_val_repeatability(loader, m, DEV, None, 0, nms_size=nms, num_points=k)
        for variant in (alone, other):
            got = train_utils.check_val_repeatability(variant, m, DEV, None, 0, nms_size=nms, num_points=k)
            assert all(np.array_equal(np.float64(a), np.float64(b)) for a, b in zip(got, full))
        last = train_utils.check_val_repeatability(loader[-1:], m, DEV, None, 0, nms_size=nms, num_points=k)
        # the loop over the one-pair functions, window leg, on the last pair's own forward
        b = loader[-1]
        ps = m(b[0][:1].to(DEV), want_logits=False)["prob"][0].cpu().numpy()
        pd = m(b[1][:1].to(DEV), want_logits=False)["prob"][0].cpu().numpy()
        _, _, want = V.gpu_loop_pair(ps, pd, b[5][0].numpy(), nms, k, "window")
    for i, key in enumerate(V.REP_KEYS):
        assert np.array_equal(np.float64(full[5 + i]), np.float64(last[5 + i])), key      # not accumulated: the last pair only
        assert np.array_equal(np.float64(full[5 + i]), np.float64(want[key])), key
    assert abs(float(full[0]) - float(last[0])) > 1.0                                     # ... while the first five are means


# ---- 5. stream order: capture and replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", V.LEGS)
def test_core_captured_in_a_graph_replays_bit_identical(g, leg):
    """Nothing inside synchronises or reads back: the core is captured with torch.cuda.graph and two replays (the second on
    other inputs copied into the captured buffers, then the first again) equal the eager calls bit for bit."""
    nms, k = int(g["meta.nms_size"]), int(g["meta.num_points"])
    names = [n for n in V.map_names(g) if g[f"{n}.prob_dst"].shape == (128, 128)]
    ps, pd, h = _stack(g, names)
    eager = [t.clone() for t in evaluate.evaluate_val_pairs(ps, pd, h, nms, k, leg=leg)]
    ps2, pd2, h2 = pd.flip(0).contiguous(), ps.flip(0).contiguous(), torch.linalg.inv(h).flip(0).contiguous()
    eager2 = [t.clone() for t in evaluate.evaluate_val_pairs(ps2, pd2, h2, nms, k, leg=leg)]
    torch.cuda.synchronize()
    a, b, c = ps.clone(), pd.clone(), h.clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(side):                                    # warm-up on the capture stream: workspaces, attributes
        evaluate.evaluate_val_pairs(a, b, c, nms, k, leg=leg)
    torch.cuda.current_stream(torch.device(DEV)).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = evaluate.evaluate_val_pairs(a, b, c, nms, k, leg=leg)
    for inputs, want in (((ps, pd, h), eager), ((ps2, pd2, h2), eager2), ((ps, pd, h), eager)):
        a.copy_(inputs[0]); b.copy_(inputs[1]); c.copy_(inputs[2])
        graph.replay()
        torch.cuda.synchronize()
        for got_t, want_t, f in zip(out, want, out._fields):
            assert np.array_equal(got_t.cpu().numpy(), want_t.cpu().numpy(), equal_nan=got_t.dtype.is_floating_point), f


# ---- 6. the split-f16 guard -------------------------------------------------------------------------------------------------
def test_flagged_chunk_is_repeated_on_the_fp32_kernels(monkeypatch):
    """A checkpoint that passes the load-time probes but leaves the f16 range on one loader image (the recipe of
    test_forward_gpu.py): the chunk is evaluated, the read finds the flag, the chunk is repeated on the fp32 kernels -- the
    result equals the fp32 model's."""
    from tests.golden import cases
    from tests.test_forward_gpu import _scaled_checkpoint_and_images
    sd, bright = _scaled_checkpoint_and_images()
    monkeypatch.delenv("BALF_FP16_STRICT", raising=False)
    monkeypatch.delenv("BALF_FP16_GUARD", raising=False)             # the default: lazy
    calm = cases.forward_input(1, 128, 128, 3)
    h = torch.tensor([[[1.0, 0.0, 4.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]]], dtype=torch.float64)
    zeros = torch.zeros((1, 1, 128, 128))
    loader = [(calm, calm.flip(-1).contiguous(), zeros, zeros, torch.linalg.inv(h), h),
              (bright, calm, zeros, zeros, torch.linalg.inv(h), h),
              (calm.flip(-2).contiguous(), calm, zeros, zeros, torch.linalg.inv(h), h)]
    ref = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    ref.load_state_dict(sd)
    ref.precision = "fp32"
    ref = ref.eval().to(DEV)
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    with torch.inference_mode():
        want = train_utils.check_val_repeatability(loader, ref, DEV, None, 0)
        with W.catch_warnings():
            W.simplefilter("error")
            m(calm.to(DEV))                                          # probes + an ordinary image: silent, split path
        assert m.effective_precision == "fp16"
        with pytest.warns(RuntimeWarning, match="left the range of its f16 halves"):
            got = train_utils.check_val_repeatability(loader, m, DEV, None, 0)
    assert m.effective_precision == "fp32"
    for a, b in zip(got, want):
        assert np.array_equal(np.float64(a), np.float64(b)), (got, want)
