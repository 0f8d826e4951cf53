"""The host side of the synthetic-pair loader (balf_amd/datasets/dataset_utils.py: generate_homography, sample_pair_geometry
...; ops.synth_pairs' argument checks) and the tests' own restatement against tests/golden/pair_synth.npz -- recorded from the
reference's functions by tests/golden/make_pair_synth_golden.py.  No GPU; only the fixture is read, never the reference tree."""
import random

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd.datasets import dataset_utils as DU
from tests import pair_synth_common as S


@pytest.fixture(scope="module")
def g():
    return S.fixture()


def _cfg(g):
    p, r, s = g["meta.geom_cfg"]
    return {"perspective": float(p), "rotation": int(r), "scale": float(s)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_sample_pair_geometry_is_the_fixtures(g):
    """Draws, windows and the composed homographies, bit for bit, for every recorded seed."""
    shape, patch = tuple(int(v) for v in g["meta.geom_shape"]), int(g["meta.geom_patch"])
    for seed in g["meta.geom_seeds"]:
        got = DU.sample_pair_geometry(shape, _cfg(g), patch, random.Random(int(seed)))
        assert tuple(got["win_src"]) == tuple(g[f"geom.{seed}.win_src"]) and tuple(got["win_dst"]) == tuple(g[f"geom.{seed}.win_dst"])
        for k in ("inv_h", "h_src_2_dst", "h_dst_2_src"):
            assert got[k].dtype == g[f"geom.{seed}.{k}"].dtype
            assert np.array_equal(_bits(got[k]), _bits(g[f"geom.{seed}.{k}"])), (seed, k)
        prod = got["h_src_2_dst"].astype(np.float64) @ got["h_dst_2_src"].astype(np.float64)
        assert np.abs(prod / prod[2, 2] - np.eye(3)).max() < 1e-5 * max(1.0, np.abs(got["h_dst_2_src"]).max()), seed


def test_windows_lie_inside_the_image():
    rng = random.Random(5)
    cfg = {"perspective": 0.2, "rotation": 25, "scale": 0.1}
    for i in range(200):
        shape = ((240, 320, 3), (200, 260, 3))[i % 2]
        patch = (64, 128)[(i // 2) % 2]
        got = DU.sample_pair_geometry(shape, cfg, patch, rng)
        for win in (got["win_src"], got["win_dst"]):
            assert 0 <= win[0] <= shape[0] - patch and 0 <= win[1] <= shape[1] - patch, (i, win)
        prod = got["h_src_2_dst"].astype(np.float64) @ got["h_dst_2_src"].astype(np.float64)
        assert np.abs(prod / prod[2, 2] - np.eye(3)).max() < 1e-5 * max(1.0, np.abs(got["h_dst_2_src"]).max()), i


def test_generate_homography_consumes_the_references_draws(g):
    """The generator's state after generate_homography is the state after the reference's get_dst_point and its four scalar
    draws; get_dst_point itself returns the reference's corners."""
    shape = tuple(int(v) for v in g["meta.geom_shape"])
    cfg = _cfg(g)
    for seed in g["meta.geom_seeds"]:
        rng = random.Random(int(seed))
        h = DU.generate_homography(shape, cfg, rng)
        assert np.array_equal(np.asarray(rng.getstate()[1], dtype=np.uint64), g[f"geom.{seed}.state"]), seed
        assert h.shape == (3, 3) and h.dtype == np.float64 and h[2, 2] == 1.0
        rng = random.Random(int(seed))
        corners = DU.get_dst_point(cfg["perspective"], shape, rng)
        assert corners.dtype == np.float32 and np.array_equal(_bits(corners), _bits(g[f"geom.{seed}.dst_point"])), seed
        rot, sc, cx, cy = (int(v) for v in g[f"geom.{seed}.scalars"])
        assert [rng.randint(-cfg["rotation"], cfg["rotation"]), rng.randint(-25, 50), rng.randint(-40, 40), rng.randint(-40, 40)] == \
            [rot, sc, cx, cy]
        # the closed forms: the four corners map where the rotation sends the perturbed ones
        rs = DU.rotation_matrix_2d((shape[1] / 2 + cx, shape[0] / 2 + cy), rot, 1.0 + cfg["scale"] * sc * 0.1)
        want = np.matmul(corners, rs.T).astype(np.float32)
        src = np.array([[0, 0, 1], [shape[1] - 1, 0, 1], [0, shape[0] - 1, 1], [shape[1] - 1, shape[0] - 1, 1]], np.float64)
        got = src @ h.T
        assert np.abs(got[:, :2] / got[:, 2:] - want).max() < 1e-6 * max(shape)


def test_restatement_reproduces_the_fixture(g):
    """tests/pair_synth_common.py against what the reference's functions recorded: heat maps, source patches, byte / 255."""
    assert np.array_equal(_bits(S.norm255(np.arange(256, dtype=np.uint8))), _bits(g["norm255"]))
    seen_src = 0
    for patch in S.PATCHES:
        for name in S.cases(patch):
            for top_k in S.TOP_KS:
                e = S.expected(patch, name, top_k)
                key = f"p{patch}.{name}.k{top_k}"
                assert np.array_equal(e[2][0], g[f"{key}.heat_src"].astype(np.float32)), key
                assert np.array_equal(e[3][0], g[f"{key}.heat_dst"].astype(np.float32)), key
            if f"p{patch}.{name}.img_src" in g:
                assert np.array_equal(_bits(S.expected(patch, name, 0)[0]), _bits(g[f"p{patch}.{name}.img_src"])), (patch, name)
                seen_src += 1
    assert seen_src == 8


def test_case_table_exercises_what_it_says():
    for patch in S.PATCHES:
        sx, sy, fx, fy = S.window_taps(patch, "frac_x")
        assert (fy == 0).all() and (fx == 24).all()
        sx, sy, fx, fy = S.window_taps(patch, "quarter_y")
        assert (fx == 0).all() and (fy == 24).all() and (sy[0] == -1).all()            # the first row's upper tap is outside
        sx, sy, fx, fy = S.window_taps(patch, "last_col")
        w = S.IMAGE_SHAPES[0][1]
        assert (sx[:, -1] == w - 1).all() and (fx[:, -1] == 8).all()                    # sx + 1 == w: outside, with weight
        e = S.expected(patch, "last_col", 0)
        assert e[1][:, :, -1].any() and e[4] > 0
        sx, sy, fx, fy = S.window_taps(patch, "rot25_half")
        assert np.abs(np.diff(sx, axis=1)).max() >= 2 and len(np.unique(fx)) > 8 and len(np.unique(fy)) > 8
        sx, sy, fx, fy = S.window_taps(patch, "mild")
        assert len(np.unique(fx)) == 32 or patch == 32
        e = S.expected(patch, "outside", 0)
        assert e[4] == 0 and not e[1].any() and not e[3].any() and e[2].any()
        e = S.expected(patch, "dups", 0)
        labels = S.fixture()["labels.dups"]
        assert len(np.unique(labels[:8, :2].astype(np.int64), axis=0)) == 4             # duplicates after truncation
        assert e[2].sum() < len(labels)                                                 # ... and points outside the window
        tie = S.fixture()["labels.mild_tie"]
        kept = S.select_k_best(tie, S.TOP_KS[0])
        cut = np.sort(tie[:, 2])[::-1][S.TOP_KS[0] - 1]
        same = np.flatnonzero(tie[:, 2] == cut)
        assert len(same) == 5 and list(np.intersect1d(kept, same)) == list(same[:3])    # the lower row indices win


def test_numpy_label_helpers(g):
    pts = g["labels.mild_tie"]
    kept = DU.select_k_best(pts, 25)
    assert len(kept) == 25 and sorted(map(tuple, kept)) == sorted(map(tuple, pts[S.select_k_best(pts, 25)]))
    assert DU.select_k_best(pts, 0) is not None and len(DU.select_k_best(pts, 0)) == len(pts) == len(DU.select_k_best(pts, 99))
    shape = S.IMAGE_SHAPES[1]
    assert np.array_equal(DU.labels_to_heatmap(kept, shape), S.heatmaps(pts, 25, shape, np.eye(3))[0])
    assert tuple(DU.get_window_point((96, 128, 3), 64, crop_type='center')) == (48.0, 64.0)
    for _ in range(20):
        r, c = DU.get_window_point((96, 128, 3), 64)
        assert 32 <= r <= 64 and 32 <= c <= 96


def test_sample_pair_geometry_refuses_an_image_smaller_than_the_window():
    with pytest.raises(ValueError):
        DU.sample_pair_geometry((60, 200, 3), {"perspective": 0.2, "rotation": 25, "scale": 0.1}, 64, random.Random(0))


def test_wrapper_argument_checks_raise():
    """ops.synth_pairs refuses host tensors before anything is launched, and the C entry its bad arguments."""
    z = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.BalfHipError):
        ops.synth_pairs(z, torch.zeros(1, dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 9), dtype=torch.float64),
                        torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), torch.zeros((0, 3)),
                        torch.zeros(2, dtype=torch.int32), 0, 32)
    l = _lib.lib()
    import ctypes as C
    fake = C.c_void_p(4096)
    args = [fake, 16, fake, fake, 1, fake, fake, fake, fake, 0, fake, 0, 32, fake, fake, fake, fake, fake, fake, 1 << 20, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return l.balf_synth_pairs(*a)

    assert l.balf_synth_pairs_workspace_bytes(1, 32) > 0 and l.balf_synth_pairs_workspace_bytes(64, 512) >= 64 * 256 * 4
    assert l.balf_synth_pairs_workspace_bytes(0, 32) == 0 and l.balf_synth_pairs_workspace_bytes(1, 0) == 0
    assert l.balf_synth_pairs_workspace_bytes(65536, 32) == 0
    for i in (0, 2, 3, 5, 6, 7, 10, 13, 14, 15, 16, 17, 18):
        assert call(**{f"a{i}": None}) == -1, i                   # null pointers
    assert call(a4=0) == -1 and call(a4=-3) == -1 and call(a4=65536) == -1          # P
    assert call(a12=0) == -1 and call(a12=-1) == -1 and call(a12=16385) == -2       # patch
    assert call(a11=-1) == -1 and call(a9=-1) == -1                                 # top_k, pts_total
    assert call(a8=None, a9=3) == -1                                                # rows without a pointer
    assert call(a19=0) == -3                                                        # workspace too small
