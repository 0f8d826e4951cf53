"""The multi-scale leg at its edges: balf_pyramid_level, balf_nms_topk_budget and balf_multiscale_merge against
the float64 references of tests/multiscale_common.py, through the C ABI into guard-banded, pre-filled buffers, at the shapes
where the kernels take another path: shrunk tiles and the large-LDS launch, refused reductions, blur radii larger than the
image, every tile phase, budgets decided from counts that are negative or exhausted, lists of 0 .. 16384 entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.benchmark_test import geometry_tools
from oracle import oracle as O
from tests import multiscale_common as MC
from tests.multiscale_common import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.fixture(scope="module", autouse=True)
def _device_checked():
    _lib.require_mi355x(torch.device(DEV))


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------
def _device_source(case):
    """-> (device tensor, kind, channels, base [B,H,W,C] fp32: the array the kernel reads)."""
    src, base = MC.case_source(case)
    ch, h, w = MC.case_channels(case), case["h_in"], case["w_in"]
    t = torch.from_numpy(src).to(DEV)
    if case["kind"].startswith("level"):
        lvl = ops.pyramid_level(t, _lib.PYR_SRC_U8, ch, h, w, 0.0, h, w)            # the previous level, written by the kernel
        _, _, top, left = arch.padded_hw(h, w)
        read_back = lvl[:, :ch, top:top + h, left:left + w].permute(0, 2, 3, 1).contiguous().cpu().numpy()
        assert np.array_equal(read_back, base)
        return lvl, _lib.PYR_SRC_LEVEL, ch, read_back
    return t, (_lib.PYR_SRC_F32 if case["kind"] == "f32rgb" else _lib.PYR_SRC_U8), ch, base


def _call_level(t, kind, ch, case, b=MC.PYR_BATCH):
    hp, wp, top, left = arch.padded_hw(case["h_out"], case["w_out"])
    dst = Guarded(b * 3 * hp * wp * 4)
    dst.view(torch.float32, (b, 3, hp, wp)).fill_(float("nan"))
    before = dst.full.clone()
    rc = _lib.lib().balf_pyramid_level(t.data_ptr(), kind, ch, b, case["h_in"], case["w_in"], float(case["sigma"]),
                                       case["h_out"], case["w_out"], dst.ptr, _stream())
    torch.cuda.synchronize()
    return rc, dst, before


def _check_case(case):
    """One accepted case -> the worst |kernel - reference| of the batch in units of 2^-24."""
    t, kind, ch, base = _device_source(case)
    rc, dst, _ = _call_level(t, kind, ch, case)
    name, ho, wo = case["name"], case["h_out"], case["w_out"]
    assert rc == 0, (name, rc)
    assert dst.intact(), f"{name}: balf_pyramid_level wrote outside its destination"
    hp, wp, top, left = arch.padded_hw(ho, wo)
    got = dst.view(torch.float32, (MC.PYR_BATCH, 3, hp, wp)).cpu().numpy()
    assert not np.isnan(got).any(), f"{name}: a padded pixel was not written"
    worst = 0.0
    for bi in range(MC.PYR_BATCH):
        ref = MC.ref_pyramid_level(base[bi], case["sigma"], ho, wo)                  # [ho,wo,ch] float64
        inner = got[bi, :, top:top + ho, left:left + wo].transpose(1, 2, 0)
        err = float(np.abs(inner[..., :ch].astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= MC.pyramid_bound(case["sigma"]), (name, bi, err / MC.ULP, MC.pyramid_bound(case["sigma"]) / MC.ULP)
        pad = got[bi].copy()
        pad[:, top:top + ho, left:left + wo] = 0
        assert not pad.any(), f"{name}: padding not zero"
        if ch == 1:
            bits = got[bi].view(np.uint32)
            assert np.array_equal(bits[0], bits[1]) and np.array_equal(bits[0], bits[2]), f"{name}: gray planes differ"
    print(f"PYR {name}: worst {worst / MC.ULP:.2f} x 2^-24, bound {MC.pyramid_bound(case['sigma']) / MC.ULP:.0f}")
    return worst / MC.ULP


@pytest.mark.parametrize("group", list(MC.PYRAMID_GROUPS))
def test_pyramid_level_vs_library_reference(group):
    worst = max(_check_case(c) for c in MC.PYRAMID_GROUPS[group])
    print(f"PYR group {group}: worst {worst:.2f} x 2^-24")


@pytest.mark.parametrize("case", MC.REFUSED_CASES, ids=[c["name"] for c in MC.REFUSED_CASES])
def test_pyramid_level_refuses_and_writes_nothing(case):
    src, _ = MC.case_source(case)
    t = torch.from_numpy(src).to(DEV)
    rc, dst, before = _call_level(t, _lib.PYR_SRC_U8, MC.case_channels(case), case)
    assert rc == ERR_ARG, (case["name"], rc)
    assert torch.equal(dst.full, before), f"{case['name']}: a refused call touched its destination"


# ---- budgeted top-K -------------------------------------------------------------------------------------------------------------------
def _budget_call(prob, top, left, h, w, border, nms, cum, k_max, taken):
    """ops.nms_topk_budget into garbage-filled guard-banded rows -> (idx, score, count, taken_after) as NumPy."""
    b = prob.shape[0]
    gi, gs, gc, gt = Guarded(b * k_max * 4), Guarded(b * k_max * 4), Guarded(b * 4), Guarded(b * 4)
    tk = gt.view(torch.int32, (b,))
    tk.copy_(torch.tensor(taken, dtype=torch.int32))
    ops.nms_topk_budget(prob, top, left, h, w, border, nms, cum, k_max, tk, gi.view(torch.int32, (b, k_max)),
                        gs.view(torch.float32, (b, k_max)), gc.view(torch.int32, (b,)))
    torch.cuda.synchronize()
    for g, name in ((gi, "idx"), (gs, "score"), (gc, "count"), (gt, "taken")):
        assert g.intact(), f"balf_nms_topk_budget wrote outside {name}"
    return (gi.view(torch.int32, (b, k_max)).cpu().numpy(), gs.view(torch.float32, (b, k_max)).cpu().numpy(),
            gc.view(torch.int32, (b,)).cpu().numpy(), tk.cpu().numpy())


def _budget_check(prob, top, left, h, w, border, nms, cum, k_max, taken, with_ops=True):
    """The budgeted call against (a) ops.nms_topk of each image alone with K = ref_budget_k, (b) the CPU oracle with that K."""
    gi, gs, gn, ta = _budget_call(prob, top, left, h, w, border, nms, cum, k_max, taken)
    pn = prob.cpu().numpy()
    ks = []
    for bi in range(prob.shape[0]):
        k = MC.ref_budget_k(cum, taken[bi], h, w, k_max)
        ks.append(k)
        idx, sc, cnt = np.full(k_max, -1, np.int32), np.zeros(k_max, np.float32), 0
        if k > 0:
            score = O.remove_borders(pn[bi, top:top + h, left:left + w], border)
            oi, os_ = O.canonical_order(*O.select_topk(O.apply_nms(score, nms), k))
            cnt = len(oi)
            idx[:cnt], sc[:cnt] = oi, os_
        assert gn[bi] == cnt <= k, (bi, gn[bi], cnt, k)
        assert np.array_equal(gi[bi], idx), bi                                      # -1 past the count
        assert np.array_equal(gs[bi].view(np.uint32), sc.view(np.uint32)), bi      # 0.0 past the count
        if k > 0 and with_ops:
            i, s, n = ops.nms_topk(prob[bi:bi + 1].contiguous(), top, left, h, w, border, nms, k)
            assert int(n[0]) == cnt
            assert np.array_equal(i[0].cpu().numpy(), idx[:k]) and np.array_equal(s[0].cpu().numpy(), sc[:k])
    assert np.array_equal(ta, np.asarray(taken, np.int64) + gn), (ta, taken, gn)
    return gi, gs, gn, ks


def _peaks(b, hp, wp, top, left, h, w, seed):
    """Distinct positive values on the even pixels of the image, zero elsewhere: with a 3 x 3 window every one survives."""
    rng = np.random.default_rng(seed)
    p = np.zeros((b, hp, wp), np.float32)
    ny, nx = (h + 1) // 2, (w + 1) // 2
    for bi in range(b):
        p[bi, top:top + h:2, left:left + w:2] = (rng.permutation(ny * nx).reshape(ny, nx) + 1.0) / (ny * nx + 1.0)
    return p


@pytest.mark.parametrize("maps", ["peaks", "zeros"])
def test_budget_k_never_exceeds_the_row(maps):
    """taken = [-3, 0, 500, 200] under cum_budget = K_max = 200: K = 200, 200, 0, 0.  Without the cap at K_max image 0 gets
    K = 203: a count of 203 for a row of 200 (both maps; 203 < next_pow2(200), so that version stays inside its LDS too)."""
    h, w, k_max = 40, 50, 200
    hp, wp, top, left = arch.padded_hw(h, w)
    p = _peaks(4, hp, wp, top, left, h, w, 1) if maps == "peaks" else np.zeros((4, hp, wp), np.float32)
    taken = [-3, 0, 500, 200]
    gi, gs, gn, ks = _budget_check(torch.from_numpy(p).to(DEV), top, left, h, w, 0, 3, 200, k_max, taken)
    assert ks == [200, 200, 0, 0]
    assert (gn <= k_max).all() and list(gn) == [200, 200, 0, 0]                     # 500 peaks / the <= 0 fallback: K each
    assert (gi[2:] == -1).all() and not gs[2:].any()


def test_budget_zero_for_the_whole_batch():
    h, w, k_max = 40, 50, 64
    hp, wp, top, left = arch.padded_hw(h, w)
    p = torch.from_numpy(_peaks(3, hp, wp, top, left, h, w, 2)).to(DEV)
    gi, gs, gn, ks = _budget_check(p, top, left, h, w, 0, 3, 0, k_max, [0, 0, 5])
    assert ks == [0, 0, 0] and not gn.any() and (gi == -1).all() and not gs.any()


def test_budget_cut_inside_a_tie_b33():
    """33 maps quantised to 8 levels, a different `taken` per image: the K-th score is shared by many survivors, and the
    lower raster index must win for a K that only the device knows."""
    b, h, w, k_max, cum, border, nms = 33, 37, 53, 64, 60, 2, 3
    hp, wp, top, left = arch.padded_hw(h, w)
    rng = np.random.default_rng(33)
    p = (np.round(rng.random((b, hp, wp), dtype=np.float32) * 8.0) / 8.0).astype(np.float32)
    taken = [(7 * bi) % 75 for bi in range(b)]                                      # 0 .. 74, all different: K from 60 down to 0
    gi, gs, gn, ks = _budget_check(torch.from_numpy(p).to(DEV), top, left, h, w, border, nms, cum, k_max, taken)
    assert max(ks) == cum and min(ks) == 0 and len(set(ks)) > 20
    in_tie = 0
    for bi in range(b):
        if ks[bi] == 0:
            continue
        nm = O.apply_nms(O.remove_borders(p[bi, top:top + h, left:left + w], border), nms).ravel()
        assert gn[bi] == ks[bi]                                                      # plateaus: far more survivors than K
        thr = gs[bi, ks[bi] - 1]
        tied = np.flatnonzero(nm == thr)
        kept = np.sort(gi[bi, :ks[bi]][gs[bi, :ks[bi]] == thr])
        if len(tied) > len(kept):
            in_tie += 1
            reach = np.flatnonzero(nm >= thr)[:ks[bi]]                               # the raster-first K that reach the threshold
            assert np.array_equal(np.sort(gi[bi, :ks[bi]]), reach)
    assert in_tie > 20


@pytest.mark.parametrize("nms,left,border", [(3, 28, 0), (8, 28, 2), (15, 21, 15), (15, 28, 15), (5, 23, 1)])
def test_budget_on_every_tile_kernel(nms, left, border):
    """The generic kernel (8), the 3 / 5 / 15 templates, and window 15 at a crop offset that is no multiple of 4 (the scalar
    kernel instead of the vector one), each under a device-decided K."""
    b, h, w, hp, wp, top, k_max = 3, 70, 90, 128, 192, 29, 150
    g = torch.Generator(device="cpu").manual_seed(nms * 100 + left)
    p = (torch.rand((b, hp, wp), generator=g) ** 4).to(DEV)
    # (taken = -40: K = 160 capped at 150; 160 < next_pow2(150), so the sizes are safe for a kernel without the cap as well)
    _, _, gn, ks = _budget_check(p, top, left, h, w, border, nms, 120, k_max, [0, 100, -40])
    assert ks == [120, 20, 150] and gn[1] <= 20 and gn[2] <= 150


def test_budget_k_max_16384():
    """K_max = 16384 on a 130 x 130 map (16900 pixels): the 128 KB sort.  Image 0 dense (window 1: every pixel survives, more
    survivors than K and than the register cache holds), image 1 all zero (the <= 0 fallback: the first 16384 raster pixels)."""
    h = w = 130
    k_max = 16384
    hp, wp, top, left = arch.padded_hw(h, w)
    rng = np.random.default_rng(16384)
    p = np.zeros((2, hp, wp), np.float32)
    p[0] = rng.permutation(hp * wp).reshape(hp, wp).astype(np.float32) / np.float32(hp * wp) + np.float32(0.001)
    gi, gs, gn, ks = _budget_check(torch.from_numpy(p).to(DEV), top, left, h, w, 0, 1, k_max, k_max, [0, 0])
    assert ks == [k_max, k_max] and list(gn) == [k_max, k_max]
    assert np.array_equal(gi[1], np.arange(k_max)) and not gs[1].any()
    flat = p[0, top:top + h, left:left + w].ravel()
    assert np.array_equal(gi[0], np.argsort(-flat.astype(np.float64), kind="stable")[:k_max])     # distinct scores


# ---- merge ----------------------------------------------------------------------------------------------------------------------------
def _diag_hms(nl, r=2.0 ** 0.5, u=1):
    return [np.linalg.inv(np.diag([1.0 / r ** (i - u), 1.0 / r ** (i - u), 1.0])) for i in range(nl)]


def _distinct(rng, population, c):
    u = np.unique(rng.integers(0, population, size=4 * c + 16))
    assert len(u) >= c
    return rng.permutation(u)[:c].astype(np.int32)


def _level_lists(rng, counts, k_max, widths, heights, scores="coarse"):
    """counts [L,B] (entries written: clip(count, 0, k_max)) -> idx / score [L,B,K_max] as the budgeted top-K writes them."""
    nl, b = counts.shape
    idx = np.full((nl, b, k_max), -1, np.int32)
    sc = np.zeros((nl, b, k_max), np.float32)
    for l in range(nl):
        for bi in range(b):
            c = int(np.clip(counts[l, bi], 0, k_max))
            ii = _distinct(rng, widths[l] * heights[l], c)
            if scores == "coarse":
                ss = (rng.integers(1, 50, size=c) / 64.0).astype(np.float32)          # many ties, within and across levels
                ss[:c // 4] = np.float32(0.25)
            elif scores == "zero":
                ss = np.zeros(c, np.float32)
            else:
                ss = np.full(c, np.float32(scores))
            o = np.lexsort((ii, -ss))
            idx[l, bi, :c], sc[l, bi, :c] = ii[o], ss[o]
    return idx, sc


def _merge_check(idx, score, count, widths, hms, n, order_yx, diagonal=True):
    """balf_multiscale_merge into a guard-banded, garbage-filled points array against ref_merge: bit-equal rows with the
    arithmetic of balf_apply_homography (and with plain NumPy for diagonal matrices), zero rows past the count."""
    nl, b, k_max = idx.shape
    ti, ts = torch.from_numpy(idx).to(DEV), torch.from_numpy(score).to(DEV)
    tc = torch.from_numpy(np.asarray(count, np.int32)).to(DEV)
    pts, cnt = Guarded(b * n * 4 * 8), Guarded(b * 4)
    w_host = (C.c_int32 * nl)(*[int(v) for v in widths])
    h_host = (C.c_double * (9 * nl))(*[float(v) for hm in hms for v in np.asarray(hm, np.float64).reshape(9)])
    rc = _lib.lib().balf_multiscale_merge(ti.data_ptr(), ts.data_ptr(), tc.data_ptr(), nl, b, k_max, w_host, h_host, n,
                                          int(order_yx), pts.ptr, cnt.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert pts.intact() and cnt.intact(), "balf_multiscale_merge wrote outside its outputs"
    gp, gc = pts.view(torch.float64, (b, n, 4)).cpu().numpy(), cnt.view(torch.int32, (b,)).cpu().numpy()
    worst = 0.0
    for bi in range(b):
        args = (idx[:, bi], score[:, bi], np.asarray(count)[:, bi], widths, hms, n, order_yx, k_max)
        ref, m = MC.ref_merge(*args, mapper=geometry_tools.apply_homography_to_points)
        assert gc[bi] == m, (bi, gc[bi], m)
        m = max(m, 0)
        assert np.array_equal(gp[bi, :m].view(np.uint64), ref.view(np.uint64)), bi
        assert not gp[bi, m:].view(np.uint64).any(), bi                              # +0.0, every bit
        ref_np, m_np = MC.ref_merge(*args)
        assert m_np == gc[bi]
        if diagonal:
            assert np.array_equal(gp[bi, :m].view(np.uint64), ref_np.view(np.uint64)), bi
        elif m:
            worst = max(worst, float((np.abs(gp[bi, :m] - ref_np) / np.maximum(np.abs(ref_np), 1.0)).max()))
            assert np.array_equal(gp[bi, :m, 3], ref_np[:, 3])
    return gp, gc, worst


WIDTHS3, HEIGHTS3 = [320, 227, 160], [240, 170, 120]


def test_merge_totals_around_powers_of_two():
    totals = [0, 1, 2, 3, 1023, 1024, 1025, 2048]
    count = np.array([[t // 3 + (t % 3 > 0), t // 3 + (t % 3 > 1), t // 3] for t in totals], np.int32).T.copy()   # [3,8]
    assert list(count.sum(0)) == totals and count.max() <= 1024
    idx, sc = _level_lists(np.random.default_rng(1), count, 1024, WIDTHS3, HEIGHTS3)
    _, gc, _ = _merge_check(idx, sc, count, WIDTHS3, _diag_hms(3), 1500, False)
    assert list(gc) == [0, 1, 2, 3, 1023, 1024, 1025, 1500]


@pytest.mark.parametrize("n", [1, 700, 16384])
def test_merge_output_length(n):
    count = np.array([[600, 2], [500, 0], [400, 3]], np.int32)                       # totals 1500 and 5
    idx, sc = _level_lists(np.random.default_rng(2), count, 1024, WIDTHS3, HEIGHTS3)
    _, gc, _ = _merge_check(idx, sc, count, WIDTHS3, _diag_hms(3), n, True)
    assert list(gc) == [min(n, 1500), min(n, 5)]


def test_merge_one_level():
    count = np.array([[37, 0, 64]], np.int32)
    idx, sc = _level_lists(np.random.default_rng(3), count, 64, [101], [77])
    _, gc, _ = _merge_check(idx, sc, count, [101], _diag_hms(1, u=0), 50, False)
    assert list(gc) == [37, 0, 50]


def test_merge_32_levels_and_the_largest_index():
    """L = 32 with entries in level 31 and the flat index 2^25 - 1 at width 8192: the key's low word uses all of its 31 bits."""
    nl, b, k_max = 32, 2, 4
    rng = np.random.default_rng(4)
    widths = [8192] * nl
    count = rng.integers(0, k_max + 1, size=(nl, b)).astype(np.int32)
    count[31] = [3, 4]
    idx, sc = _level_lists(rng, count, k_max, widths, [4096] * nl)
    idx[31, 0, 0] = idx[31, 1, 2] = 2 ** 25 - 1
    idx[0, 0, 0] = 2 ** 25 - 1
    count[0, 0] = max(count[0, 0], 1)
    sc[31, 0, 0] = sc[0, 0, 0] = np.float32(0.25)                                    # tied with level 0's largest index
    hms = [np.diag([1.0 + 0.03125 * l, 1.0 + 0.03125 * l, 1.0]) for l in range(nl)]
    gp, gc, _ = _merge_check(idx, sc, count, widths, hms, 128, False)
    assert gc[0] == count[:, 0].sum() and gc[1] == count[:, 1].sum()
    x31 = 8191.0 * (1.0 + 0.03125 * 31)
    assert (gp[0, :gc[0], 0] == x31).any() and (gp[1, :gc[1], 0] == x31).any()


@pytest.mark.parametrize("scores", ["zero", 0.5])
def test_merge_score_ties_order_by_level_then_index(scores):
    """Every score +0.0 (what the <= 0 fallback writes at several levels at once) / one positive value everywhere."""
    count = np.array([[20, 0], [64, 5], [0, 7], [33, 64]], np.int32)
    widths, heights = [64, 45, 32, 23], [48, 34, 24, 17]
    idx, sc = _level_lists(np.random.default_rng(5), count, 64, widths, heights, scores=scores)
    hms = [np.diag([float(l + 1), float(l + 1), 1.0]) for l in range(4)]            # x' = (l + 1) x: the level shows in the row
    gp, gc, _ = _merge_check(idx, sc, count, widths, hms, 100, False)
    for bi in range(2):
        want = [((ii % widths[l]) * (l + 1.0), (ii // widths[l]) * (l + 1.0))
                for l in range(4) for ii in np.sort(idx[l, bi, :count[l, bi]])][:100]
        assert [tuple(r) for r in gp[bi, :gc[bi], :2]] == want


def test_merge_clamps_the_input_counts():
    """Counts of -5 and K_max + 7 are read as 0 and K_max.  Every slot of every row is filled, so a count taken as it stands
    would bring in entries of the next row."""
    k_max = 64
    full = np.full((3, 2), k_max, np.int32)
    idx, sc = _level_lists(np.random.default_rng(6), full, k_max, WIDTHS3, HEIGHTS3)
    count = np.array([[k_max + 7, 30], [-5, k_max], [10, 0]], np.int32)
    _, gc, _ = _merge_check(idx, sc, count, WIDTHS3, _diag_hms(3), 150, False)
    assert list(gc) == [k_max + 10, 30 + k_max]


@pytest.mark.parametrize("extra", [0, 1])
def test_merge_at_the_capacity(extra):
    """Counts (8192, 8192, 0): 16384 entries, exactly the cap, the 128 KB sort.  One more entry: count -1 and zero rows for that
    image, the other image of the batch as if alone."""
    k_max, n = 8192, 16384
    count = np.array([[8192, 100], [8192, 0], [extra, 50]], np.int32)
    idx, sc = _level_lists(np.random.default_rng(7), np.array([[8192, 100], [8192, 0], [1, 50]]), k_max, WIDTHS3, HEIGHTS3)
    gp, gc, _ = _merge_check(idx, sc, count, WIDTHS3, _diag_hms(3), n, False)
    assert list(gc) == [-1 if extra else 16384, 150]
    if extra:
        assert not gp[0].any()


@pytest.mark.parametrize("order_yx", [False, True])
def test_merge_projective_homographies(order_yx):
    """General matrices (h[6], h[7] != 0): the rows are bit-equal with balf_apply_homography, the one function both run
    (csrc/homography.h); against plain NumPy they agree to rounding (the device contracts a*b + c into one operation, NumPy
    does not), which is the contract DESIGN.md 7b states.  1e-12 relative: ~4500 units of 2^-52 for a form of ~20 operations
    on well-conditioned matrices (|det| ~ 1, denominator in [0.9, 1.2])."""
    count = np.array([[120, 3], [80, 0], [64, 128]], np.int32)
    idx, sc = _level_lists(np.random.default_rng(8), count, 128, WIDTHS3, HEIGHTS3)
    hms = [np.array([[0.71, 0.013, 2.5], [-0.021, 0.69, -1.25], [1.5e-4, -2.5e-4, 1.0]]),
           np.array([[1.02, -0.04, 0.3], [0.05, 0.97, 4.0], [-3e-4, 2e-4, 1.01]]),
           np.array([[1.39, 0.02, -7.0], [0.03, 1.43, 5.5], [4e-4, 6e-4, 0.98]])]
    _, gc, worst = _merge_check(idx, sc, count, WIDTHS3, hms, 256, order_yx, diagonal=False)
    print(f"MERGE projective order_yx={order_yx}: worst relative difference to NumPy {worst:.3g}")
    assert list(gc) == [256, 131]
    assert worst <= 1e-12
