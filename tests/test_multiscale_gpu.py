"""Multi-scale extraction on the GPU (balf_amd/multiscale.py; balf_pyramid_level, balf_nms_topk_budget and
balf_multiscale_merge in include/balf_hip.h) against NumPy restatements of the protocol written here."""
import os

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, multiscale as MS, ops, pipeline
from balf_amd.benchmark_test import geometry_tools
from balf_amd.model import get_model
from balf_amd.utils import synth
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def models():
    out = {}
    for prec in ("fp32", "fp16"):
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(synth.synthetic_state_dict(cases.WEIGHT_SEED))
        m.precision = prec
        out[prec] = m.eval().to(DEV)
    return out


# ---- restatement of the pyramid (float64) ----------------------------------------------------------------------------------
def np_blur(img, sigma):
    t = MS.gaussian_taps(sigma)
    r = (len(t) - 1) // 2
    p = np.pad(img, ((r, r), (0, 0), (0, 0)), mode="symmetric")       # half-sample symmetric = scipy's 'reflect'
    img = sum(t[k] * p[k:k + img.shape[0]] for k in range(2 * r + 1))
    p = np.pad(img, ((0, 0), (r, r), (0, 0)), mode="symmetric")
    return sum(t[k] * p[:, k:k + img.shape[1]] for k in range(2 * r + 1))


def np_resize(img, ho, wo):
    def axis(n_in, n_out):
        s = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, s - i0
    y0, y1, ly = axis(img.shape[0], ho)
    x0, x1, lx = axis(img.shape[1], wo)
    ly, lx = ly[:, None, None], lx[None, :, None]
    top = (1 - lx) * img[y0][:, x0] + lx * img[y0][:, x1]
    bot = (1 - lx) * img[y1][:, x0] + lx * img[y1][:, x1]
    return (1 - ly) * top + ly * bot


def np_pyramid(img, plan):
    """img [H,W,C] float64 (level U) -> the levels [h_i,w_i,C] float64."""
    u = plan.upsampled_levels
    lv = [None] * len(plan.shapes)
    lv[u] = img
    for i in range(u):
        lv[i] = np_resize(img, *plan.shapes[i])
    for i in range(u + 1, len(plan.shapes)):
        lv[i] = np_resize(np_blur(lv[i - 1], plan.sigma), *plan.shapes[i])
    return lv


@pytest.mark.parametrize("case", ["rgb_480x640_u8", "gray_1080x1920_u8", "rgb_333x517_u8", "rgb_333x517_float",
                                  "gray_301x402_u8_two_up"])
def test_pyramid_levels_vs_restatement(case):
    rng = np.random.default_rng(len(case))
    kind, hw = case.split("_")[0], case.split("_")[1]
    h, w = map(int, hw.split("x"))
    u = 2 if case.endswith("two_up") else 1
    b = 2
    shape = (b, h, w) if kind == "gray" else (b, h, w, 3)
    im8 = (np.clip(rng.normal(128, 60, shape), 0, 255)).astype(np.uint8)
    if case.endswith("float"):
        imf = rng.random((b, h, w, 3))                    # float64 in [0, 1): cast to float32 on the device
        src = torch.from_numpy(imf).to(DEV)
        base = imf.astype(np.float32)
    else:
        src = torch.from_numpy(im8).to(DEV)
        rgb = im8 if kind == "rgb" else np.repeat(im8[..., None], 3, axis=-1)
        base = (rgb.astype(np.float64) / 255.0).astype(np.float32)
    plan = MS.pyramid_plan(h, w, 1500, np.sqrt(2), 5, u, 15)
    levels = ops.build_pyramid(src, plan.shapes, u, plan.sigma)
    torch.cuda.synchronize()
    # level U is the forward's prepared input, bit for bit (padding included)
    prepared = pipeline.pad_batch(base.astype(np.float64)).numpy()
    assert np.array_equal(levels[u].cpu().numpy(), prepared)
    for bi in range(b):
        ref = np_pyramid(base[bi].astype(np.float64), plan)
        for i, (hh, ww) in enumerate(plan.shapes):
            hp, wp, top, left = plan.padded[i]
            got = levels[i][bi].cpu().numpy()
            assert got.shape == (3, hp, wp)
            inner = got[:, top:top + hh, left:left + ww].transpose(1, 2, 0)
            err = np.abs(inner - ref[i]).max()
            assert err <= 1e-5, (case, bi, i, err)
            pad = got.copy()
            pad[:, top:top + hh, left:left + ww] = 0
            assert not pad.any(), (case, i, "padding not zero")
            if kind == "gray":
                assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- budgeted top-K ----------------------------------------------------------------------------------------------------------
def test_budgeted_topk_matches_host_decided_k():
    g = torch.Generator(device="cpu").manual_seed(7)
    b, k_max = 3, 200
    geoms, probs = [], []
    for hh, ww, hp, wp in ((100, 130, 128, 192), (70, 90, 128, 128), (6, 7, 64, 64), (40, 50, 64, 64)):
        geoms.append((hh, ww, (hp - hh) // 2, (wp - ww) // 2))
        probs.append(torch.rand((b, hp, wp), generator=g) ** 4)
    # level 1: image 0 has 3 positive peaks only (fewer than its share of 60: the later levels get the rest), image 1 is all
    # zero (the <= 0 fallback); level 2 (6x7 = 42 pixels): all zero for images 0 and 1, image 0's K of 87 clamped at h*w;
    # level 3: image 1 has taken its whole budget (K = 0)
    probs[1][0].zero_()
    for (y, x) in ((20, 30), (40, 60), (50, 20)):
        probs[1][0, geoms[1][2] + y, geoms[1][3] + x] = 0.5
    probs[1][1].zero_()
    probs[2][0].zero_()
    probs[2][1].zero_()
    probs = [p.to(DEV) for p in probs]
    cum = [60, 120, 150, 150]
    borders = [15, 15, 0, 15]
    taken = torch.zeros(b, dtype=torch.int32, device=DEV)
    got = []
    for p, (hh, ww, top, left), c, bd in zip(probs, geoms, cum, borders):
        i, s, n = ops.nms_topk_budget(p, top, left, hh, ww, bd, 15, c, k_max, taken)
        got.append((i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()))
    # expectation: K from the counts read back on the host, then ops.nms_topk on each image alone
    tk = [0] * b
    for li, (p, (hh, ww, top, left), c, bd) in enumerate(zip(probs, geoms, cum, borders)):
        idx = np.full((b, k_max), -1, np.int32)
        sc = np.zeros((b, k_max), np.float32)
        cnt = np.zeros(b, np.int32)
        for bi in range(b):
            k = min(c - tk[bi], hh * ww)
            if k > 0:
                i, s, n = ops.nms_topk(p[bi:bi + 1].contiguous(), top, left, hh, ww, bd, 15, k)
                idx[bi, :k], sc[bi, :k], cnt[bi] = i[0].cpu().numpy(), s[0].cpu().numpy(), int(n[0])
                tk[bi] += int(n[0])
        gi, gs, gn = got[li]
        assert np.array_equal(gn, cnt), (li, gn, cnt)
        assert np.array_equal(gi, idx), li
        assert np.array_equal(gs.view(np.uint32), sc.view(np.uint32)), li
    assert np.array_equal(taken.cpu().numpy(), np.array(tk, np.int32))
    # the constructed cases did what they are for
    c0 = got[0][2]
    k1 = 120 - int(c0[1])
    assert got[1][2][0] == 3                                                          # fewer survivors than the share
    assert got[1][2][1] == k1 and np.array_equal(got[1][0][1, :k1], np.arange(k1))    # <= 0 fallback: first K raster pixels
    assert 150 - int(c0[0]) - 3 > 42                                                  # image 0's K at level 2 ...
    assert got[2][2][0] == 42 and np.array_equal(got[2][0][0, :42], np.arange(42))    # ... clamped at h*w
    assert got[2][2][1] == 30                                                         # 150 - 120
    assert got[3][2][1] == 0 and (got[3][0][1] == -1).all()                           # K = 0
    assert got[3][2][0] > 0                                                           # image 0's unused share passed down


# ---- merge -----------------------------------------------------------------------------------------------------------------
def np_merge(idx, score, count, widths, hms, n, order_yx):
    rows = []
    for l in range(idx.shape[0]):
        for j in range(count[l]):
            rows.append((-float(score[l, j]), l, int(idx[l, j]), score[l, j]))
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    rows = rows[:n]
    out = np.zeros((len(rows), 4))
    for r, (_, l, i, s) in enumerate(rows):
        x, y = i % widths[l], i // widths[l]
        p = geometry_tools.apply_homography_to_points(np.array([[x, y, 1.0, s]], np.float64), hms[l])[0]
        out[r] = p
    if order_yx and len(out):
        out[:, [0, 1]] = out[:, [1, 0]]
    return out


@pytest.mark.parametrize("order_yx", [False, True])
def test_merge_vs_restatement(order_yx):
    rng = np.random.default_rng(3)
    plan = MS.pyramid_plan(240, 320, num_points=300)
    nl, b, k_max, n = len(plan.shapes), 2, 300, 300
    idx = np.full((nl, b, k_max), -1, np.int32)
    score = np.zeros((nl, b, k_max), np.float32)
    count = np.zeros((nl, b), np.int32)
    ties = np.float32(0.25)
    for bi in range(b):
        for l, (hh, ww) in enumerate(plan.shapes):
            c = [plan.point_level[l], plan.point_level[l] // 2][bi]
            ii = rng.choice(hh * ww, size=c, replace=False).astype(np.int32)
            ss = (rng.integers(1, 50, size=c) / 64.0).astype(np.float32)          # coarse scores: many ties
            ss[: c // 4] = ties                                                    # equal scores across levels
            o = np.lexsort((ii, -ss))
            idx[l, bi, :c], score[l, bi, :c], count[l, bi] = ii[o], ss[o], c
    widths = [s[1] for s in plan.shapes]
    pts, cnt = ops.multiscale_merge(torch.from_numpy(idx).to(DEV), torch.from_numpy(score).to(DEV),
                                    torch.from_numpy(count).to(DEV), widths, plan.homographies, n, order_yx)
    pts, cnt = pts.cpu().numpy(), cnt.cpu().numpy()
    for bi in range(b):
        ref = np_merge(idx[:, bi], score[:, bi], count[:, bi], widths, plan.homographies, n, order_yx)
        assert cnt[bi] == len(ref) == min(n, int(count[:, bi].sum()))
        assert np.array_equal(pts[bi, :cnt[bi]].view(np.uint64), ref.view(np.uint64)), bi
        assert not pts[bi, cnt[bi]:].any()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _composed(model, images_u8, plan, border=15, nms=15, order_yx=False):
    """build_pyramid -> per-level detect_batch with the K read back per image -> host merge."""
    levels = ops.build_pyramid(images_u8, plan.shapes, plan.upsampled_levels, plan.sigma)
    b, n = images_u8.shape[0], plan.num_points
    widths = [s[1] for s in plan.shapes]
    out = []
    for bi in range(b):
        taken = 0
        li_idx = np.full((len(levels), n), -1, np.int32)
        li_sc = np.zeros((len(levels), n), np.float32)
        li_cnt = np.zeros(len(levels), np.int32)
        for l, x in enumerate(levels):
            hh, ww = plan.shapes[l]
            k = min(plan.cum_budget[l] - taken, hh * ww)
            if k <= 0:
                continue
            i, s, c, _ = pipeline.detect_batch(model, x[bi:bi + 1].contiguous(), hh, ww, border, nms, k)
            c = int(c[0])
            li_idx[l, :c], li_sc[l, :c], li_cnt[l] = i[0, :c].cpu().numpy(), s[0, :c].cpu().numpy(), c
            taken += c
        out.append(np_merge(li_idx, li_sc, li_cnt, widths, plan.homographies, n, order_yx))
    return out


@pytest.mark.parametrize("gray", [True, False])
def test_end_to_end_matches_composition(models, gray):
    m = models["fp16"]
    rng = np.random.default_rng(11)
    h, w = 240, 320
    ims = np.stack([synth.synthetic_gray_u8(h, w, s) for s in range(3)])
    if not gray:
        ims = np.stack([ims, np.roll(ims, 7, axis=1), 255 - ims], axis=-1)
    ims = np.ascontiguousarray(ims)
    x = torch.from_numpy(ims).to(DEV)
    plan = MS.pyramid_plan(h, w, num_points=400)
    with torch.inference_mode():
        pts, cnt = MS.detect_batch_multiscale_u8(m, x, num_points=400)
        pts, cnt = pts.cpu().numpy(), cnt.cpu().numpy()
        ref = _composed(m, x, plan)
        for bi in range(3):
            assert cnt[bi] == len(ref[bi]) and 0 < cnt[bi] <= 400
            assert np.array_equal(pts[bi, :cnt[bi]].view(np.uint64), ref[bi].view(np.uint64)), bi
            alone, ca = MS.detect_batch_multiscale_u8(m, x[bi:bi + 1].contiguous(), num_points=400)
            assert int(ca[0]) == cnt[bi]
            assert np.array_equal(alone[0].cpu().numpy().view(np.uint64), pts[bi].view(np.uint64)), bi
    del rng


def test_float_input_matches_u8_input(models):
    m = models["fp32"]
    ims = np.stack([np.stack([synth.synthetic_gray_u8(200, 260, s)] * 3, -1) for s in range(2)])
    with torch.inference_mode():
        p8, c8 = MS.detect_batch_multiscale_u8(m, torch.from_numpy(ims).to(DEV), num_points=300)
        pf, cf = MS.detect_batch_multiscale(m, torch.from_numpy(ims / 255.0).to(DEV), num_points=300)
    assert np.array_equal(c8.cpu().numpy(), cf.cpu().numpy())
    assert np.array_equal(p8.cpu().numpy(), pf.cpu().numpy())


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_no_pyramid_equals_extract_detections(models, precision):
    m = models[precision]
    im = synth.gray_to_rgb_norm(synth.synthetic_gray_u8(300, 410, 5))
    with torch.inference_mode():
        ref, _ = pipeline.extract_detections(im, m, DEV, nms_size=15, num_points=25, border_size=15)
        got = MS.extract_multiscale_detections(im, m, DEV, nms_size=15, num_points=25, border_size=15, pyramid_levels=0,
                                               upsampled_levels=0)
    assert got.shape == ref.shape == (25, 4)
    assert np.array_equal(got[:, [0, 1, 3]], ref[:, [0, 1, 3]])
    rad = geometry_tools.apply_homography_to_points(ref, np.eye(3))[:, 2]
    assert np.array_equal(got[:, 2], rad)


def test_graph_capture_replays_on_new_inputs(models):
    m = models["fp16"]
    h, w = 200, 260
    mk = lambda s: torch.from_numpy(np.stack([synth.synthetic_gray_u8(h, w, s + i) for i in range(2)])).to(DEV)
    static = mk(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.inference_mode():
        with torch.cuda.stream(side):
            for _ in range(2):
                MS.detect_batch_multiscale_u8(m, static, num_points=300)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = MS.detect_batch_multiscale_u8(m, static, num_points=300)
        for seed in (10, 20):
            new = mk(seed)
            static.copy_(new)
            graph.replay()
            got = (out[0].clone(), out[1].clone())
            ref = MS.detect_batch_multiscale_u8(m, new, num_points=300)
            torch.cuda.synchronize()
            assert torch.equal(got[1], ref[1])
            assert torch.equal(got[0], ref[0])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_caller_on_photographs(models, precision):
    f = np.load(os.path.join(G, "natural.npz"))
    m = models[precision]
    for name in ("im1", "im2"):
        im = f[name + ".u8"] / 255.0
        with torch.inference_mode():
            xy = MS.extract_multiscale_detections(im, m, DEV)
            yx = MS.extract_multiscale_detections(im, m, DEV, order_coord="yxsr")
        assert m.effective_precision == precision
        assert xy.dtype == np.float64 and xy.ndim == 2 and xy.shape[1] == 4
        assert 0 < len(xy) <= 1500
        assert np.all(np.diff(xy[:, 3]) <= 0)
        assert np.array_equal(yx[:, [1, 0, 2, 3]], xy)
        h, w = im.shape[:2]
        assert xy[:, 0].min() >= 0 and xy[:, 0].max() < w + 2 and xy[:, 1].min() >= 0 and xy[:, 1].max() < h + 2
        assert len(np.unique(xy[:, 2])) > 1                   # points from several levels (radius = s_i)
