"""The host side of the training task's photometric distortion (balf_amd/datasets/dataset_utils.py: sample_photometric,
sample_pair_geometry's photometric_rng; the argument checks of ops.photometric_u8 / ops.synth_train_pairs and of the two C
entries) and the tests' restatement (tests/photometric_common.py) against tests/golden/photometric.npz -- recorded from the
reference's functions by tests/golden/make_photometric_golden.py.  No GPU; only the fixtures are read, never the reference."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd.datasets import dataset_utils as DU
from tests import pair_synth_common as S
from tests import photometric_common as PC


@pytest.fixture(scope="module")
def fx():
    return PC.fixture()


class _Logged:
    """A generator that logs its calls the way the recorder logged the reference's."""

    def __init__(self, rng):
        self.rng, self.log = rng, []

    def randint(self, *a):
        v = self.rng.randint(*a)
        self.log.append((0.0, float(a[0]), float(a[1]) if len(a) > 1 else np.nan, float(v)))
        return v

    def uniform(self, lo, hi):
        v = self.rng.uniform(lo, hi)
        self.log.append((1.0, float(lo), float(hi), float(v)))
        return v


def _state(st):
    return np.append(st[1], st[2]).astype(np.uint32)


def test_sample_photometric_makes_the_references_draws(fx):
    """Per seed: the same calls with the same arguments in the same order (so the brightness value is the hue's range when that
    branch fired, and the second alpha exists only with the first), the same values, and the generator left in the same state
    -- from the global np.random and from a RandomState."""
    assert DU.perms == tuple(map(tuple, fx["perms"])) == PC.PERMS
    seen_quirk = False
    for s in fx["meta.seeds"]:
        want, log = fx[f"draws.{s}.params"], fx[f"draws.{s}.log"]
        np.random.seed(int(s))
        got = DU.sample_photometric()
        assert np.array_equal(got["params"].view(np.uint64), want[:5].view(np.uint64)) and got["perm"] == int(want[5]), s
        assert got["params"].dtype == np.float64 and isinstance(got["perm"], int)
        assert np.array_equal(_state(np.random.get_state()), fx[f"draws.{s}.state"]), s
        rs = np.random.RandomState(int(s))
        logged = _Logged(rs)
        again = DU.sample_photometric(logged)
        assert np.array_equal(again["params"], got["params"]) and again["perm"] == got["perm"]
        assert np.array_equal(np.asarray(logged.log), log, equal_nan=True), s
        assert np.array_equal(_state(rs.get_state()), fx[f"draws.{s}.state"]), s
        bright, contrast, _, hue, _ = fx[f"draws.{s}.fired"]
        if bright and hue:                                           # the quirk: uniform(-brightness, brightness)
            row = log[[i for i in range(len(log)) if log[i, 0] == 1][1 + contrast + int(fx[f"draws.{s}.fired"][2])]]
            assert row[1] == -want[0] and row[2] == want[0] and abs(row[2]) != 18.0
            seen_quirk = True
        if not contrast:
            assert want[1] == 1.0 and want[4] == 1.0
    assert seen_quirk
    assert list(fx["cast_u8"]) == [68, 103, 255]                     # what the recorder's platform made of 324.5, 359.9, 255.9


def test_restatement_gives_the_recorded_images(fx):
    n = 0
    for s in fx["meta.seeds"]:
        p, perm = PC.draws_to_params(fx[f"draws.{s}.params"])
        for k in range(int(fx["meta.images_per_seed"])):
            im = fx[f"img.{s}.{k}.in"]
            assert np.array_equal(im, PC.fixture_image(int(s), k))
            assert np.array_equal(PC.distort(im, p, perm), fx[f"img.{s}.{k}.out"]), (s, k)
            assert np.array_equal(PC.distort(im[..., ::-1], p, perm, blue_idx=2), fx[f"img.{s}.{k}.out"][..., ::-1]), (s, k)
            n += 1
        assert np.array_equal(fx[f"rgb.{s}"], fx[f"img.{s}.0.out"][..., ::-1])
    assert n == 64


def test_neutral_parameters_leave_only_the_hsv_round_trip():
    """Steps 1, 3, 4, 6 and 7 are the identity at their neutral values; the 8-bit HSV round trip in between is not (the
    reference makes it whatever fired): gray pixels survive it, many colours do not."""
    v = np.arange(256, dtype=np.uint8)
    gray = np.stack([v, v, v], axis=-1)[None]
    assert np.array_equal(PC.distort(gray, PC.NEUTRAL, 0), gray)
    lattice = np.stack(np.meshgrid(v[::5], v[::5], v[::5], indexing="ij"), axis=-1).reshape(1, -1, 3)
    out = PC.distort(lattice, PC.NEUTRAL, 0)
    assert np.array_equal(out, PC.hsv2bgr_u8(PC.bgr2hsv_u8(lattice)))
    assert (out != lattice).any()                                   # (so "neutral" is NOT "the image itself")
    for perm, order in enumerate(PC.PERMS):
        assert np.array_equal(PC.distort(gray * 0 + lattice[:, :256], PC.NEUTRAL, perm), out[:, :256][..., list(order)])


def _counting(monkeypatch):
    calls = []
    real = DU.generate_homography
    monkeypatch.setattr(DU, "generate_homography", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_every_homography_draw_consumes_one_photometric_set(monkeypatch):
    """A 64 x 64 window in a 70 x 72 image: most destination windows leave the image and the pair is redrawn.  The geometry
    is the one drawn without photometric_rng; the generator has advanced by one sample_photometric per homography draw, and
    the set returned is the last one."""
    cfg = {"perspective": 0.2, "rotation": 25, "scale": 0.1}
    shape, patch = (70, 72, 3), 64
    redrawn = 0
    for seed in range(6):
        calls = _counting(monkeypatch)
        plain = DU.sample_pair_geometry(shape, cfg, patch, random.Random(seed))
        n = len(calls)
        assert "photometric" not in plain and sorted(plain) == ["h_dst_2_src", "h_src_2_dst", "inv_h", "win_dst", "win_src"]
        prng = np.random.RandomState(100 + seed)
        got = DU.sample_pair_geometry(shape, cfg, patch, random.Random(seed), photometric_rng=prng)
        assert len(calls) == 2 * n
        for k in plain:
            assert np.array_equal(np.asarray(plain[k]), np.asarray(got[k])), (seed, k)
        twin = np.random.RandomState(100 + seed)
        sets = [DU.sample_photometric(twin) for _ in range(n)]
        assert np.array_equal(got["photometric"]["params"], sets[-1]["params"]) and got["photometric"]["perm"] == sets[-1]["perm"]
        assert np.array_equal(_state(prng.get_state()), _state(twin.get_state())), seed
        redrawn += n > 1
    assert redrawn >= 3


def test_default_geometry_is_still_the_recorded_one():
    g = S.fixture()
    p, r, s = g["meta.geom_cfg"]
    cfg = {"perspective": float(p), "rotation": int(r), "scale": float(s)}
    shape, patch = tuple(int(v) for v in g["meta.geom_shape"]), int(g["meta.geom_patch"])
    for seed in g["meta.geom_seeds"]:
        rng, twin = random.Random(int(seed)), random.Random(int(seed))
        got = DU.sample_pair_geometry(shape, cfg, patch, rng)
        assert sorted(got) == ["h_dst_2_src", "h_src_2_dst", "inv_h", "win_dst", "win_src"]
        assert tuple(got["win_src"]) == tuple(g[f"geom.{seed}.win_src"]) and tuple(got["win_dst"]) == tuple(g[f"geom.{seed}.win_dst"])
        for k in ("inv_h", "h_src_2_dst", "h_dst_2_src"):
            assert got[k].tobytes() == g[f"geom.{seed}.{k}"].tobytes(), (seed, k)
        DU.sample_pair_geometry(shape, cfg, patch, twin, photometric_rng=np.random.RandomState(0))
        assert rng.getstate() == twin.getstate()                    # the random module's draws do not depend on the task


def test_numpy_helpers():
    a = np.array([[[-3.0, 100.5, 300.0], [255.0, 0.0, 256.0]]])
    b = a.copy()
    assert DU.check_margins(b) is b and np.array_equal(b, [[[0.0, 100.5, 255.0], [255.0, 0.0, 255.0]]])
    c = a.copy()
    assert DU.check_margins(c, axis=2) is c and np.array_equal(c, [[[-3.0, 100.5, 255.0], [255.0, 0.0, 255.0]]])
    assert np.array_equal(DU.swap_channels(a, DU.perms[3]), a[:, :, [1, 2, 0]])


def test_python_entry_points_check_their_arguments_and_have_no_cpu_path():
    z = torch.zeros(12, dtype=torch.uint8)
    off, sizes = torch.zeros(1, dtype=torch.int64), torch.tensor([[2, 2]], dtype=torch.int32)
    prm, perm = torch.tensor([PC.NEUTRAL], dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.photometric_u8(z, off, sizes, prm, perm)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.synth_train_pairs(z, off, sizes, torch.zeros((1, 9), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.int32),
                              torch.zeros((1, 2), dtype=torch.int32), torch.zeros((0, 3)), torch.zeros(2, dtype=torch.int32), 0, 2,
                              prm, perm)
    with pytest.raises(ValueError):
        DU.photometric_u8(np.zeros((4, 4), np.uint8), DU.sample_photometric(np.random.RandomState(0)))
    with pytest.raises(ValueError):
        DU.bgr_distorsion(np.zeros((4, 4, 3), np.float32))


def test_c_entry_points_refuse_bad_arguments_before_launching():
    l = _lib.lib()
    fake = C.c_void_p(4096)
    assert len(_lib.PROTOTYPES["balf_photometric_u8"][1]) == 10 and len(_lib.PROTOTYPES["balf_synth_train_pairs"][1]) == 23
    assert not [n for n in _lib.PROTOTYPES if "photometric" in n or "train_pairs" in n
                if n.endswith(("_workspace_bytes", "_saved_bytes"))]

    photo = [fake, 48, fake, fake, 1, fake, fake, 0, fake, None]

    def call_photo(**kw):
        a = list(photo)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return l.balf_photometric_u8(*a)

    for i in (0, 2, 3, 5, 6, 8):
        assert call_photo(**{f"a{i}": None}) == -1, i
    assert call_photo(a4=0) == -1 and call_photo(a4=-1) == -1 and call_photo(a4=65536) == -1            # B
    for blue in (1, 3, -1, 255):
        assert call_photo(a7=blue) == -1, blue

    pairs = [fake, 16, fake, fake, 1, fake, fake, fake, fake, 0, fake, 0, 32, fake, fake, fake, fake, fake, fake, 1 << 20, fake, fake,
             None]

    def call_pairs(**kw):
        a = list(pairs)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return l.balf_synth_train_pairs(*a)

    for i in (0, 2, 3, 5, 6, 7, 10, 13, 14, 15, 16, 17, 18, 20, 21):
        assert call_pairs(**{f"a{i}": None}) == -1, i                # null pointers, the two new ones included
    assert call_pairs(a4=0) == -1 and call_pairs(a4=65536) == -1                                         # P
    assert call_pairs(a12=0) == -1 and call_pairs(a12=16385) == -2                                       # patch
    assert call_pairs(a11=-1) == -1 and call_pairs(a9=-1) == -1 and call_pairs(a8=None, a9=3) == -1      # top_k, pts_total
    assert call_pairs(a19=l.balf_synth_pairs_workspace_bytes(1, 32) - 1) == -3                           # the shared workspace
