"""The references of the multi-scale edge tests checked against each other, without a GPU (tests/multiscale_common.py): the
library reference against the NumPy restatement, the fp32 emulation of the kernel against the derived bound, the merge and budget
references against brute force, and the case list against the branches of the host's tile choice."""
import numpy as np
import pytest

from tests import multiscale_common as MC

ALL = MC.PYRAMID_CASES


# ---- the NumPy restatement of tests/test_multiscale_gpu.py (restated: that module needs a GPU to import its fixtures) ----------
def np_blur(img, sigma):
    r = MC.blur_radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-0.5 * k * k / (sigma * sigma))
    t = t / t.sum()
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


@pytest.fixture(scope="module")
def refs():
    """name -> (base [H,W,C] fp32 of image 0, float64 reference): computed once, left unchanged."""
    out = {}
    for c in ALL:
        base = MC.case_source(c, b=1)[1][0]
        ref = MC.ref_pyramid_level(base, c["sigma"], c["h_out"], c["w_out"])
        ref.setflags(write=False)
        out[c["name"]] = (base, ref)
    return out


@pytest.mark.parametrize("group", list(MC.PYRAMID_GROUPS))
def test_reference_agrees_with_restatement(refs, group):
    worst = 0.0
    for c in MC.PYRAMID_GROUPS[group]:
        base, ref = refs[c["name"]]
        x = base.astype(np.float64)
        if MC.blur_radius(c["sigma"]) > 0:
            x = np_blur(x, c["sigma"])
        got = np_resize(x, c["h_out"], c["w_out"])
        assert got.shape == ref.shape == (c["h_out"], c["w_out"], MC.case_channels(c))
        err = float(np.abs(got - ref).max()) / MC.ULP
        worst = max(worst, err)
        assert err <= 1.0, (c["name"], err)
    print(f"{group}: scipy/torch reference vs restatement, worst {worst:.3g} x 2^-24")


@pytest.mark.parametrize("group", list(MC.PYRAMID_GROUPS))
def test_fp32_emulation_within_bound(refs, group):
    worst = 0.0
    for c in MC.PYRAMID_GROUPS[group]:
        base, ref = refs[c["name"]]
        emu = MC.fp32_emulation_level(base, c["sigma"], c["h_out"], c["w_out"])
        err = float(np.abs(emu.astype(np.float64) - ref).max())
        worst = max(worst, err / MC.pyramid_bound(c["sigma"]))
        print(f"{c['name']}: fp32 emulation {err / MC.ULP:.2f} x 2^-24, bound {MC.pyramid_bound(c['sigma']) / MC.ULP:.0f}")
        assert err <= MC.pyramid_bound(c["sigma"]), (c["name"], err / MC.ULP)
    print(f"{group}: worst ratio to the bound {worst:.3f}")


def test_identity_blur_and_gray_reference():
    x = np.random.default_rng(0).random((9, 11, 1), dtype=np.float32)
    a = MC.ref_pyramid_level(x, 0.1, 9, 11)                     # int(4 * 0.1 + 0.5) = 0 and same size: the source itself
    assert np.array_equal(a, x.astype(np.float64))
    assert np.array_equal(MC.ref_pyramid_level(x[..., 0], 0.0, 5, 7), MC.ref_pyramid_level(x, 0.0, 5, 7))
    assert np.array_equal(MC.fp32_emulation_level(x, 0.1, 9, 11), x)


# ---- merge reference ----------------------------------------------------------------------------------------------------------------
def brute_merge(idx, score, count, widths, hms, n, order_yx, k_max):
    rows = []
    for l in range(idx.shape[0]):
        for j in range(min(max(int(count[l]), 0), k_max)):
            rows.append((-float(score[l, j]), l, int(idx[l, j])))
    if len(rows) > min(idx.shape[0] * k_max, 16384):
        return np.zeros((0, 4)), -1
    rows.sort()
    rows = rows[:n]
    out = np.zeros((len(rows), 4))
    for r, (ns, l, i) in enumerate(rows):
        out[r] = MC.np_homography_points(np.array([[i % widths[l], i // widths[l], 1.0, -ns]]), hms[l])[0]
    if order_yx and len(out):
        out[:, [0, 1]] = out[:, [1, 0]]
    return out, len(rows)


def _lists(rng, nl, k_max, counts, widths, scores):
    idx = np.full((nl, k_max), -1, np.int32)
    sc = np.zeros((nl, k_max), np.float32)
    for l, c in enumerate(np.clip(counts, 0, k_max)):
        idx[l, :c] = np.sort(rng.choice(widths[l] * 50, size=c, replace=False))
        sc[l, :c] = scores(c)
        o = np.lexsort((idx[l, :c], -sc[l, :c]))
        idx[l, :c], sc[l, :c] = idx[l, :c][o], sc[l, :c][o]
    return idx, sc


@pytest.mark.parametrize("scores", ["ties_across_levels", "all_zero", "distinct"])
@pytest.mark.parametrize("order_yx", [False, True])
def test_ref_merge_vs_brute_force(scores, order_yx):
    rng = np.random.default_rng(5)
    nl, k_max, widths = 4, 40, [64, 45, 32, 23]
    hms = [np.diag([s, s, 1.0]) for s in (0.5, 1.0, 2.0 ** 0.5, 2.0)]
    hms[2] = np.array([[1.1, 0.02, 3.0], [-0.03, 0.9, 1.0], [1e-4, -2e-4, 1.0]])
    gen = {"ties_across_levels": lambda c: (rng.integers(1, 4, size=c) / 4.0).astype(np.float32),
           "all_zero": lambda c: np.zeros(c, np.float32),
           "distinct": lambda c: rng.random(c, dtype=np.float32)}[scores]
    for counts, n in (([40, 17, 0, 5], 30), ([40, 17, 0, 5], 100), ([-5, 47, 1, 0], 41), ([0, 0, 0, 0], 7)):
        idx, sc = _lists(rng, nl, k_max, counts, widths, gen)
        got, m = MC.ref_merge(idx, sc, counts, widths, hms, n, order_yx, k_max)
        want, mw = brute_merge(idx, sc, counts, widths, hms, n, order_yx, k_max)
        assert m == mw == min(n, int(np.clip(counts, 0, k_max).sum()))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_ref_merge_overflow():
    idx = np.zeros((2, 16384), np.int32)
    sc = np.zeros((2, 16384), np.float32)
    hms, widths = [np.eye(3)] * 2, [8, 8]
    assert MC.ref_merge(idx, sc, [16384, 0], widths, hms, 4, False, 16384)[1] == 4
    rows, m = MC.ref_merge(idx, sc, [16384, 1], widths, hms, 4, False, 16384)
    assert m == -1 and rows.shape == (0, 4)
    assert MC.ref_merge(idx, sc, [99999, -1], widths, hms, 4, False, 16384)[1] == 4          # clamped first


# ---- budget reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cum,taken,h,w,k_max,want", [
    (200, -3, 40, 50, 200, 200),          # a count below zero never makes K longer than a row
    (200, 0, 40, 50, 200, 200),
    (200, 500, 40, 50, 200, 0),           # taken > cum_budget
    (200, 200, 40, 50, 200, 0),
    (0, 0, 40, 50, 200, 0),               # cum_budget = 0
    (0, -7, 40, 50, 200, 7),
    (150, 20, 6, 7, 300, 42),             # h*w < budget
    (150, 120, 6, 7, 300, 30),
    (16384, -2 ** 31, 130, 130, 16384, 16384),
])
def test_ref_budget_k(cum, taken, h, w, k_max, want):
    assert MC.ref_budget_k(cum, taken, h, w, k_max) == want


# ---- the case list reaches every branch of the tile choice ----------------------------------------------------------------------
def test_case_list_covers_the_tile_choice():
    chosen = {c["name"]: MC.tile_choice(c["h_in"], c["w_in"], c["sigma"], c["h_out"], c["w_out"]) for c in ALL}
    assert all(ty >= 1 for ty, _ in chosen.values()), "an accepted case is refused by the restated tile choice"
    assert {ty for ty, _ in chosen.values()} == {8, 4, 2, 1}
    assert chosen["ty1_r8_60k"] == (1, 60192) and chosen["ty4_r2"][0] == 4 and chosen["ty2_r4"][0] == 2
    assert chosen["ty8_r0_over48k"][0] == 8 and chosen["ty8_r0_over48k"][1] > 48 * 1024
    lds = [b for _, b in chosen.values()]
    assert min(lds) <= 48 * 1024 < max(lds) <= 64 * 1024
    assert any(ty == 8 and b <= 48 * 1024 for ty, b in chosen.values())
    # the refusals: one source column past the largest accepted reduction, with R = 8 and with R = 0
    ref = {c["name"]: c for c in MC.REFUSED_CASES}
    for fits, past, r in (("fits_r8", "past_r8", 8), ("fits_r0", "past_r0", 0)):
        f, p = next(c for c in ALL if c["name"] == fits), ref[past]
        assert MC.blur_radius(f["sigma"]) == MC.blur_radius(p["sigma"]) == r
        assert (p["h_in"], p["h_out"], p["w_out"], p["w_in"]) == (f["h_in"], f["h_out"], f["w_out"], f["w_in"] + 1)
        assert chosen[fits][0] == 1 and MC.tile_choice(p["h_in"], p["w_in"], p["sigma"], p["h_out"], p["w_out"]) == (0, None)
    # the limits the header states: ceil(63 in/out) <= 412 (R = 8), 1163 (R = 2), 2727 (R = 0)
    for r, sigma, lim in ((8, 2.0, 412), (2, 0.5, 1163), (0, 0.0, 2727)):
        assert MC.tile_choice(1, lim, sigma, 1, 63)[0] == 1 and MC.tile_choice(1, lim + 1, sigma, 1, 63) == (0, None)
    # radii: every accepted radius edge, and the sigma refusals are refused for their radius / value, not their size
    assert {MC.blur_radius(c["sigma"]) for c in ALL} >= {0, 2, 4, 8}
    assert MC.blur_radius(2.1) == 8 and MC.blur_radius(2.2) == 9 and MC.blur_radius(0.1) == 0
    kinds = [c["kind"] for c in ALL if not c["name"].startswith("sweep")]
    assert all(kinds.count(k) >= 2 for k in ("u8gray", "u8rgb", "f32rgb", "level1", "level3"))
