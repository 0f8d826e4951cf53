"""Host side of the multi-scale extraction (balf_amd/multiscale.py): the pyramid plan, its argument checks and the blur taps.
No GPU needed."""
import numpy as np
import pytest

from balf_amd import _lib, arch
from balf_amd.multiscale import gaussian_taps, pyramid_plan


def test_default_plan_1080p():
    p = pyramid_plan(1080, 1920)
    assert p.point_level == [755, 377, 188, 94, 47, 23, 11]
    assert sum(p.point_level) == 1495
    assert p.cum_budget == list(np.cumsum(p.point_level))
    assert p.shapes == [(1527, 2715), (1080, 1920), (764, 1358), (541, 961), (383, 680), (271, 481), (192, 341)]
    assert p.padded == [arch.padded_hw(h, w) for h, w in p.shapes]
    padded_px = sum(hp * wp for hp, wp, _, _ in p.padded)
    assert round(padded_px / (1088 * 1920), 2) == 4.07
    r = np.sqrt(2)
    for i, (s, hm) in enumerate(zip(p.scales, p.homographies)):
        assert s == r ** (i - 1)
        np.testing.assert_array_equal(hm, np.linalg.inv(np.diag([1 / s, 1 / s, 1.0])))
    assert p.sigma == 2 * r / 6


def test_default_plan_vga():
    p = pyramid_plan(480, 640)
    assert p.shapes[0] == (679, 905) and p.shapes[1] == (480, 640) and p.shapes[-1] == (86, 114)
    assert len(p.shapes) == 7
    assert round(sum(hp * wp for hp, wp, _, _ in p.padded) / (512 * 640), 2) == 4.24


def test_small_levels_end_the_pyramid():
    p = pyramid_plan(100, 120, num_points=100, border_size=15)
    # 141x170, 100x120, 71x85, 51x61, 37x44, then 27x32 (27 <= 30): not built
    assert p.shapes == [(141, 170), (100, 120), (71, 85), (51, 61), (37, 44)]
    q = pyramid_plan(100, 120, num_points=100, border_size=40)
    assert q.shapes == [(141, 170), (100, 120)]                # 71 <= 80: that level and every later one dropped
    r2 = np.sqrt(2) ** 2
    tmp = r2 + 1.0
    assert q.point_level == [int(100 * r2 / tmp), int(100 / tmp)]
    with pytest.raises(ValueError):
        pyramid_plan(60, 60, border_size=40, upsampled_levels=0)      # not even level 0 is large enough


def test_no_pyramid_is_the_single_scale_call():
    p = pyramid_plan(200, 300, num_points=25, pyramid_levels=0, upsampled_levels=0)
    assert p.shapes == [(200, 300)] and p.point_level == [25] and p.scales == [1.0]
    np.testing.assert_array_equal(p.homographies[0], np.eye(3))


@pytest.mark.parametrize("kw", [dict(scale_factor_levels=1.0), dict(scale_factor_levels=0.5), dict(pyramid_levels=-1),
                                dict(upsampled_levels=-1), dict(num_points=_lib.MAX_TOPK + 1), dict(num_points=0)])
def test_argument_checks(kw):
    with pytest.raises(ValueError):
        pyramid_plan(480, 640, **kw)


def test_gaussian_taps_match_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    for sigma in (2 * np.sqrt(2) / 6, 2 * 1.5 / 6, 2 * 2.0 / 6):
        t = gaussian_taps(sigma)
        rad = (len(t) - 1) // 2
        imp = np.zeros(4 * rad + 9)
        imp[len(imp) // 2] = 1.0
        ref = nd.gaussian_filter1d(imp, sigma, mode="reflect", truncate=4.0)
        c = len(imp) // 2
        np.testing.assert_allclose(t, ref[c - rad:c + rad + 1][::-1], rtol=0, atol=1e-15)
        assert abs(ref.sum() - 1.0) < 1e-12 and np.all(ref[:c - rad] == 0)
    assert len(gaussian_taps(2 * np.sqrt(2) / 6)) == 5          # radius 2 for the default sqrt(2)
