"""The references of the descriptor-leg edge tests, tested on the CPU (no GPU): tests/descriptor_common.py against
oracle.match_smnn and oracle.extract_patches on easy inputs, and the caps the GPU file relies on -- at least 95 % of the
matcher rows of every near-duplicate case are decided (so the GPU comparison leaves out at most 5 %), and the fp32 level
formula of the library picks the level the fp64 reference picks for every patch case."""
import functools

import numpy as np
import pytest
import torch

from balf_amd import _lib
from oracle import oracle
from tests import descriptor_common as DC


@functools.lru_cache(maxsize=None)
def _near_ref(sigma, scale):
    d1, d2, _, _ = DC.near_duplicate_case(sigma, scale)
    return DC.MatchRef(d1, d2, DC.NEAR_TH)


@pytest.mark.parametrize("n1,n2,th", [(60, 90, 0.95), (33, 16, 0.8), (2, 2, 0.99), (1, 5, 0.99), (5, 1, 0.99)])
def test_match_reference_equals_oracle_on_easy_inputs(n1, n2, th):
    rng = np.random.default_rng(n1 + n2)
    d1, d2 = DC.unit_rows(n1, 1), DC.unit_rows(n2, 2)
    m = min(n1, n2) // 2
    if m:
        noisy = d1[:m] + 0.15 * rng.standard_normal((m, 128)).astype(np.float32)
        d2[rng.permutation(n2)[:m]] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    ref = DC.MatchRef(d1, d2, th)
    od, oi = oracle.match_smnn(torch.from_numpy(d1), torch.from_numpy(d2), th)
    assert np.array_equal(oi.numpy().reshape(-1, 2), ref.idx)
    if len(od):
        assert np.abs(od.numpy() - ref.dist).max() < 1e-6                 # the oracle rounds its distances to fp32
        assert len(ref.idx) >= m // 2
    assert ref.check(ref.idx, ref.dist, note=lambda s: None)[1] == 0      # the reference passes its own check, all decided


def test_match_reference_tie_and_nan_rules():
    """lowest index on exact ties (th = 1.0 lets the tied row through); a NaN row is nobody's neighbour, as in the oracle"""
    # the NaN half runs at th = 0.9 on the same rows: the tied rows have ratio 1 there and match nothing
    d1, d2 = DC.tie_case()
    ref = DC.MatchRef(d1, d2, 1.0)
    got = {tuple(r) for r in ref.idx.tolist()}
    for i, (ja, jb) in enumerate(DC.TIE_PAIRS):
        assert np.array_equal(d2[ja], d2[jb]) and ja < jb
        assert (i, ja) in got and (i, jb) not in got
        assert ref.rows.d1[i] == ref.rows.d2[i] > 0.0 and ref.rows.ratio[i] == 1.0
    swapped = {tuple(r) for r in DC.MatchRef(d2, d1, 1.0).idx.tolist()}
    assert swapped == {(j, i) for i, j in got}
    # (oracle.match_smnn is no reference here: torch.topk leaves the order among exactly equal distances open)
    bad = d2.copy()
    bad[20] = np.nan
    clean, withnan = DC.MatchRef(d1, d2, 0.9), DC.MatchRef(d1, bad, 0.9)
    _, oi = oracle.match_smnn(torch.from_numpy(d1), torch.from_numpy(bad), 0.9)
    assert np.array_equal(oi.numpy().reshape(-1, 2), withnan.idx)
    assert [r for r in clean.idx.tolist() if r[1] != 20] == withnan.idx.tolist()


@pytest.mark.parametrize("sigma,scale", DC.NEAR_CASES)
def test_decided_share_of_the_near_duplicate_cases(sigma, scale):
    """The cap the GPU test relies on: the accuracy contract decides at least 95 % of the rows (and of the columns)."""
    ref = _near_ref(sigma, scale)
    rows, cols = ref.decided_share()
    n_match = sum(ref.pair_state(int(i), int(j)) == "match" for i, j in ref.idx)
    print(f"sigma {sigma} scale {scale}: decided rows {rows:.3f} columns {cols:.3f}; {len(ref.idx)} matches, {n_match} decided")
    assert rows >= 0.95 and cols >= 0.95
    assert n_match >= 0.9 * DC.NEAR_SOURCES                                # the planted pairs are what gets compared
    # the planted rows are the hard ones: their two nearest are the near-duplicates, 128 sigma^2 and 288 sigma^2 apart
    d1, d2, src, dst = DC.near_duplicate_case(sigma, scale)
    assert np.array_equal(np.sort(np.stack([dst[0::2], dst[1::2]], 1), 1),
                          np.sort(np.argsort(DC.dist2_f64(d1[src], d2), axis=1)[:, :2], 1))


def test_fp32_expansion_stays_inside_the_contract():
    """Provenance of delta: d^2 = |a|^2 + |b|^2 - 2 a.b with every operation in fp32 (NumPy's summation order) against the
    fp64 differences, on the near-duplicate cases: the worst error is below 16 * 2^-24 * (|a| + |b|)^2."""
    for sigma, scale in DC.NEAR_CASES:
        d1, d2, _, _ = DC.near_duplicate_case(sigma, scale)
        na, nb = (d1 * d1).sum(1, dtype=np.float32), (d2 * d2).sum(1, dtype=np.float32)
        emu = (na[:, None] + nb[None, :]) - np.float32(2.0) * (d1 @ d2.T)
        assert emu.dtype == np.float32
        bound = DC.DELTA_C * (np.sqrt(na.astype(np.float64))[:, None] + np.sqrt(nb.astype(np.float64))[None, :]) ** 2
        rel = np.abs(emu.astype(np.float64) - DC.dist2_f64(d1, d2)) / bound
        print(f"sigma {sigma} scale {scale}: worst fp32 error / delta = {rel.max():.3f}")
        assert rel.max() < 1.0


def _library_level(h, w, scale):
    """the level the library picks, read off the workspace it asks for (a host function: no GPU needed)"""
    nbytes = _lib.lib().balf_extract_patches_batch_workspace_bytes(1, h, w, float(scale))
    hits = [lv for lv in range(0, 8) if DC.patch_workspace_bytes(1, h, w, lv) == nbytes]
    assert hits, f"{nbytes} workspace bytes for {h}x{w} at scale {scale} match no number of levels"
    return len(DC.level_sizes(h, w, hits[0]))


@pytest.mark.parametrize("h,w,scale,what", DC.PATCH_CASES)
def test_level_choice_fp32_equals_fp64(h, w, scale, what):
    lv = DC.level_f64(h, w, scale)
    assert DC.level_f32(h, w, scale) == lv, f"{h}x{w} scale {scale!r}: fp32 and fp64 level formulas differ"
    assert _library_level(h, w, scale) == len(DC.level_sizes(h, w, lv))


def test_level_cases_are_what_they_claim():
    made = {(h, w, s): len(DC.level_sizes(h, w, DC.level_f64(h, w, s))) for h, w, s, _ in DC.PATCH_CASES}
    assert DC.level_f64(160, 200, 300.0) == 4 and made[(160, 200, 300.0)] == 3          # the early stop
    assert made[(128, 128, 130.0)] == 3 and made[(131, 203, 130.0)] == 3 and made[(64, 200, 130.0)] == 1
    assert [made[(96, 96, s)] for s in (16.0, 32.0, 64.0)] == [0, 1, 2]
    below, above = DC.PATCH_CASES[-2][2], DC.PATCH_CASES[-1][2]
    assert below < 32.0 < above and made[(96, 96, below)] == 0 and made[(96, 96, above)] == 1
    # the workspace of the early-stop shape: three levels, not four
    assert DC.patch_workspace_bytes(3, 160, 200, 4) == 256 + 96000 + 24064 + 6144


def test_patch_reference_vs_fp32_oracle():
    """Both are references.  The largest difference over all cases is the record the GPU tolerance is built from
    (descriptor_common.PATCH_F32_ORACLE_VS_F64; measured 1.262e-5, at 96x96 scale 16 -- level 0 of uint8 noise, where a
    coordinate ulp meets the largest contrast)."""
    worst = 0.0
    for h, w, scale, what in DC.PATCH_CASES:
        gray, xy = DC.patch_image(h, w), DC.patch_points(h, w)
        ref = DC.extract_patches_f64(gray, xy, scale)
        o32 = oracle.extract_patches(torch.from_numpy(gray.astype(np.float32) / 255.0), torch.from_numpy(xy),
                                     float(np.float32(scale)))[:, 0].numpy()
        err = float(np.abs(ref - o32).max())
        print(f"{h}x{w} scale {scale!r} ({what}): fp32 oracle vs fp64 reference {err:.3e}")
        assert ref.shape == (DC.PATCH_POINTS, 32, 32) and ref.min() >= 0.0 and ref.max() <= 1.0
        worst = max(worst, err)
    print(f"worst {worst:.4e}")
    assert worst <= DC.PATCH_F32_ORACLE_VS_F64
    assert worst > DC.PATCH_F32_ORACLE_VS_F64 / 4.0          # the record is a measurement, not a generous guess


def test_patch_points_cover_the_edges():
    for h, w, _, _ in DC.PATCH_CASES:
        xy = DC.patch_points(h, w)
        assert xy.shape == (DC.PATCH_POINTS, 2) and xy.dtype == np.float32
        assert {(0.0, 0.0), (w - 1.0, h - 1.0), (-5.0, -5.0), (w + 3.0, h + 7.0)} <= {tuple(p) for p in xy.tolist()}
        assert np.any(xy[:, 0] % 1 == 0.5)


def test_gray_formula_equals_pil():
    from PIL import Image
    rgb = np.random.default_rng(5).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    rgb[0, :6] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 127, 129]]
    assert np.array_equal(DC.gray_formula(rgb), np.array(Image.fromarray(rgb).convert("L")))
