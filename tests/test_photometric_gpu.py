"""The training task's photometric distortion on the GPU (include/balf_hip.h: balf_photometric_u8, balf_synth_train_pairs;
ops.photometric_u8, ops.synth_train_pairs, datasets.dataset_utils.bgr_distorsion, SyntheticPairs(photometric_seed=...))
against tests/photometric_common.py's restatement of the definition and tests/golden/photometric.npz, recorded from the
reference's functions.  Every comparison is EXACT: bytes, and float32 patches as bits.  Only fixtures are read here."""
import functools
import random

import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets import dataset_utils as DU
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.stage4_train import TrainableStage4
from balf_amd.utils import synth, train_utils
from tests import pair_synth_common as S
from tests import photometric_common as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1 << 20
BRIGHT = ((36.0, 1.0, 1.0, 0.0, 1.0), 0)    # a black pixel becomes (36, 36, 36): the zero border must NOT
BORDER_CASES = ("shift_int", "outside", "last_col", "quarter_y")     # windows whose taps leave the image
PATCHES = (5, 16, 37)                       # rows of 1.25, 4 and 9.25 four-pixel stores


@pytest.fixture(scope="module")
def fx():
    return PC.fixture()


@functools.lru_cache(maxsize=None)
def fixture_sets():
    """Eight recorded parameter sets: the seeds with the most branches fired (ties: the lower seed)."""
    g = PC.fixture()
    seeds = sorted((int(s) for s in g["meta.seeds"]), key=lambda s: -int(g[f"draws.{s}.fired"].sum()))[:8]
    sets = [PC.draws_to_params(g[f"draws.{s}.params"]) for s in seeds]
    assert len({p.tobytes() for p, _ in sets}) == 8
    return tuple((tuple(p), perm) for p, perm in sets)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(b):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}


def _host(out):
    return [t.cpu().numpy() for t in out]


def _labels():
    g = S.fixture()
    return {str(n): g[f"labels.{n}"] for n in g["meta.cases"]}


# ---- balf_photometric_u8 ----------------------------------------------------------------------------------------------------
def _pack_images(images, sets):
    nbytes = [im.size for im in images]
    return {"packed": np.concatenate([im.reshape(-1) for im in images]),
            "offsets": np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64),
            "sizes": np.asarray([im.shape[:2] for im in images], np.int32),
            "params": np.asarray([p for p, _ in sets], np.float64), "perm": np.asarray([q for _, q in sets], np.int32)}


def _photo(b, blue_idx, out=None):
    d = _dev(b)
    return ops.photometric_u8(d["packed"], d["offsets"], d["sizes"], d["params"], d["perm"], blue_idx, out=out)


def _split(flat, images):
    out, at = [], 0
    for im in images:
        out.append(flat[at:at + im.size].reshape(im.shape))
        at += im.size
    return out


def test_all_byte_triples_with_neutral_parameters():
    """Every (b, g, r) once, as one 4096 x 4096 image: the tables and both conversions over their whole domain."""
    v = np.arange(256, dtype=np.uint8)
    im = np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(4096, 4096, 3))
    got = _photo(_pack_images([im], [(PC.NEUTRAL, 0)]), 0).cpu().numpy().reshape(im.shape)
    want = PC.distort(im, PC.NEUTRAL, 0)
    bad = np.flatnonzero((got != want).any(axis=-1).reshape(-1))
    assert bad.size == 0, (bad.size, im.reshape(-1, 3)[bad[:5]], got.reshape(-1, 3)[bad[:5]], want.reshape(-1, 3)[bad[:5]])


EXTREMES = (((36.0, 1.0, 1.0, 0.0, 1.0), 0), ((-36.0, 1.0, 1.0, 0.0, 1.0), 0), ((0.0, 0.5, 1.0, 0.0, 0.5), 0),
            ((0.0, 1.5, 1.0, 0.0, 1.5), 0), ((0.0, 1.0, 1.0, 36.0, 1.0), 0), ((0.0, 1.0, 1.0, -36.0, 1.0), 0),
            ((36.0, 1.5, 1.5, -36.0, 0.5), 3), ((-36.0, 0.5, 0.5, 36.0, 1.5), 4))


@pytest.mark.parametrize("blue_idx", (0, 2))
def test_lattice_under_recorded_extreme_and_permuted_parameters(blue_idx):
    """The 64^3 lattice of every fourth byte value as a 512 x 512 image per parameter set, all sets in one call."""
    v = np.arange(0, 256, 4, dtype=np.uint8)
    lattice = np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(512, 512, 3))
    sets = list(fixture_sets()) + list(EXTREMES) + [((10.0, 1.1, 1.2, -7.0, 0.9), q) for q in range(6)]
    images = [lattice] * len(sets)
    got = _split(_photo(_pack_images(images, sets), blue_idx).cpu().numpy(), images)
    for i, (p, q) in enumerate(sets):
        want = PC.distort(lattice, p, q, blue_idx)
        assert np.array_equal(got[i], want), (i, p, q, int((got[i] != want).sum()))
    assert not np.array_equal(got[-1], got[-6])                                   # the permutations do differ


def test_odd_sizes_unaligned_offsets_in_place_and_the_refusals(fx):
    """Images of 1 x 1, 7 x 9, 5 x 3 and 16 x 16 back to back: offsets that are no multiple of four (the byte path) and pixel
    counts that are no multiple of a thread's four; in place; an image outside the buffer is not written, a perm outside the
    table gives a black image, and neither disturbs its neighbours."""
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((1, 1), (7, 9), (5, 3), (16, 16), (3, 4), (2, 2))]
    sets = list(fixture_sets()[:6])
    b = _pack_images(images, sets)
    assert any(o % 4 for o in b["offsets"]) and any(o % 4 == 0 for o in b["offsets"][1:])
    want = [PC.distort(im, p, q, 2) for im, (p, q) in zip(images, sets)]
    got = _split(_photo(b, 2).cpu().numpy(), images)
    for i in range(len(images)):
        assert np.array_equal(got[i], want[i]), i
    packed = torch.from_numpy(b["packed"]).to(DEV)
    d = _dev(b)
    same = ops.photometric_u8(packed, d["offsets"], d["sizes"], d["params"], d["perm"], 2, out=packed)
    assert same.data_ptr() == packed.data_ptr() and np.array_equal(packed.cpu().numpy(), np.concatenate([w.reshape(-1) for w in want]))
    b["perm"][1], b["perm"][4] = 6, -1
    b["offsets"][3] = b["packed"].size - 16 * 16 * 3 + 1                         # one byte too far
    out = torch.full((b["packed"].size,), 0xA5, dtype=torch.uint8, device=DEV)
    got = _split(_photo(b, 2, out=out).cpu().numpy(), images)
    for i in (0, 2, 5):
        assert np.array_equal(got[i], want[i]), i
    assert not got[1].any() and not got[4].any() and (got[3] == 0xA5).all()


def test_bgr_distorsion_under_a_seed_is_the_recorded_output(fx):
    for s in fx["meta.seeds"]:
        for k in range(int(fx["meta.images_per_seed"])):
            np.random.seed(int(s))
            got = DU.bgr_distorsion(fx[f"img.{s}.{k}.in"])
            assert got.dtype == np.uint8 and np.array_equal(got, fx[f"img.{s}.{k}.out"]), (s, k)
        np.random.seed(int(s))
        assert np.array_equal(DU.bgr_photometric_to_rgb(fx[f"img.{s}.0.in"]), fx[f"rgb.{s}"]), s


# ---- balf_synth_train_pairs -------------------------------------------------------------------------------------------------
def _sets_for(names):
    sets = fixture_sets()
    return [BRIGHT if n in BORDER_CASES else sets[i % len(sets)] for i, n in enumerate(names)]


def _train_batch(patch, names, sets):
    b = S.pack_batch(patch, names, _labels())
    b["params"], b["perm"] = np.asarray([p for p, _ in sets], np.float64), np.asarray([q for _, q in sets], np.int32)
    return b


def _run_train(d, top_k, patch, out=None):
    return ops.synth_train_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"],
                                 d["pts_offsets"], top_k, patch, d["params"], d["perm"], out=out)


def _run_plain(d, top_k, patch):
    return ops.synth_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"], d["pts_offsets"],
                           top_k, patch)


@functools.lru_cache(maxsize=None)
def expected(patch, name, top_k, params, perm):
    """crop(warp_perspective_u8(restated_distortion(image), inv_h)) and the rest of pair_np (callers must not write it)."""
    c = S.cases(patch)[name]
    im = S.images()[c["image"]]
    e = S.pair_np(im, _labels()[name], top_k, c["inv_h"], c["win_src"], c["win_dst"], patch)
    warped = S.crop(S.warp_perspective_u8(PC.distort(im, params, perm, blue_idx=2), c["inv_h"]), c["win_dst"], patch)
    return e[0], np.ascontiguousarray(S.norm255(warped).transpose(2, 0, 1)), e[2], e[3], int(warped.max())


def _assert_pair(got, i, want, what):
    for k in range(4):
        assert np.array_equal(_bits(got[k][i]), _bits(want[k])), (what, k)
    assert int(got[4][i]) == want[4], (what, int(got[4][i]), want[4])


@pytest.mark.parametrize("patch", PATCHES)
def test_every_case_against_the_restatement(patch):
    """All recorded geometries in one call, windows at the corners and taps outside the image included; three of them again as
    a call of P = 3.  The cases that look outside run with brightness +36: their border stays 0 where distort(0) is 36."""
    names = list(S.cases(patch))
    sets = _sets_for(names)
    assert PC.distort(np.zeros((1, 1, 3), np.uint8), *BRIGHT).min() == 36
    got = _host(_run_train(_dev(_train_batch(patch, names, sets)), 25, patch))
    for i, n in enumerate(names):
        _assert_pair(got, i, expected(patch, n, 25, *sets[i]), (patch, n))
    i = names.index("shift_int")                                     # dst(x, y) = src(x - 20, y + 7), window flush left and bottom
    assert not got[1][i][:, :, :min(20, patch)].any() and not got[1][i][:, -min(7, patch):, :].any()
    assert patch <= 20 or got[1][i][:, :-7, 20:].min() > 0          # inside: at least 36 before the HSV round trip
    assert not got[1][names.index("outside")].any() and int(got[4][names.index("outside")]) == 0
    three = ["mild", "rot25_half", "last_col"]
    sets3 = [fixture_sets()[1], fixture_sets()[4], BRIGHT]
    got3 = _host(_run_train(_dev(_train_batch(patch, three, sets3)), 0, patch))
    for i, n in enumerate(three):
        _assert_pair(got3, i, expected(patch, n, 0, *sets3[i]), (patch, n, "P=3"))


@pytest.mark.parametrize("patch", PATCHES)
def test_fused_call_equals_the_two_call_composition(patch):
    """balf_photometric_u8 (R, G, B order) on a copy of each pair's image, then balf_synth_pairs on the distorted copies: every
    output of the fused call, bit for bit -- but the source patch, which the composition cuts from the distorted copy and the
    training task from the image itself (balf_synth_pairs' own)."""
    names = list(S.cases(patch))
    sets = _sets_for(names)
    b = _train_batch(patch, names, sets)
    ims = S.images()
    own = [ims[S.cases(patch)[n]["image"]] for n in names]           # one copy per pair: each has its own parameters
    b["packed"] = np.concatenate([im.reshape(-1) for im in own])
    b["offsets"] = np.concatenate([[0], np.cumsum([im.size for im in own])[:-1]]).astype(np.int64)
    d = _dev(b)
    fused = _host(_run_train(d, 25, patch))
    plain = _host(_run_plain(d, 25, patch))
    d2 = dict(d, packed=ops.photometric_u8(d["packed"], d["offsets"], d["sizes"], d["params"], d["perm"], 2))
    two = _host(_run_plain(d2, 25, patch))
    for k in (1, 2, 3, 4):
        assert np.array_equal(fused[k].view(np.uint32), two[k].view(np.uint32)), k
    for k in (0, 2, 3):                                              # the source side never sees the distortion
        assert np.array_equal(fused[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert not np.array_equal(fused[1], plain[1]) and not np.array_equal(two[0], plain[0])


def test_neutral_parameters():
    """Neutral parameters leave the 8-bit HSV round trip, which the reference makes whatever fired and which is not the
    identity on colours (test_photometric_host.py): on GRAY images, which survive it, all five outputs are balf_synth_pairs'
    own; on the coloured images every output but the destination patch and its maximum is, and those are the restatement's."""
    patch, names = 16, list(S.cases(16))
    sets = [(PC.NEUTRAL, 0)] * len(names)
    b = _train_batch(patch, names, sets)
    d = _dev(b)
    got, plain = _host(_run_train(d, 25, patch)), _host(_run_plain(d, 25, patch))
    for k in (0, 2, 3):
        assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), k
    for i, n in enumerate(names):
        _assert_pair(got, i, expected(patch, n, 25, PC.NEUTRAL, 0), n)
    gray = np.concatenate([np.repeat(im[:, :, :1], 3, axis=2).reshape(-1) for im in S.images()])
    d = _dev(dict(b, packed=gray))
    got, plain = _host(_run_train(d, 25, patch)), _host(_run_plain(d, 25, patch))
    for k in range(5):
        assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert got[1].any()


def test_edge_pairs_do_not_disturb_their_neighbours():
    """A perm outside the table: an all-zero destination patch and dst_max = -1, the source side as ever.  An image outside
    the buffer: all zero, -1.  A singular inv_h: a zero destination patch with dst_max = 0.  The pairs between them: as in
    the restatement."""
    patch = 16
    names = ["mild", "rot25_half", "mild", "dups", "mild", "one_label", "mild"]
    sets = [fixture_sets()[i] for i in range(len(names))]
    b = _train_batch(patch, names, sets)
    b["perm"][0], b["perm"][6] = 6, -1
    b["offsets"][2] = b["packed"].size - 100
    b["inv_h"][4] = np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    d = _dev(b)
    got, plain = _host(_run_train(d, 0, patch)), _host(_run_plain(d, 0, patch))
    for i in (1, 3, 5):
        _assert_pair(got, i, expected(patch, names[i], 0, *sets[i]), (i, names[i]))
    for k in (0, 2, 3):                                              # the source patch and both heat maps of EVERY pair
        assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), k
    for i in (0, 2, 4, 6):
        assert not got[1][i].any(), i
    assert list(got[4][[0, 2, 4, 6]]) == [-1, -1, 0, -1]
    assert got[0][0].any() and not got[0][2].any() and got[0][4].any()


def _guarded(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((2 * GUARD + n,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def test_guard_bands_around_every_output():
    """Each output is written at its documented size, all of it and nothing else: 1 MiB of 0xA5 on both sides stays, no
    element inside keeps the pattern."""
    patch = 37
    names = ["mild", "last_col", "identity_br"]
    sets = _sets_for(names)
    shapes = ((3, 3, patch, patch), (3, 3, patch, patch), (3, 1, patch, patch), (3, 1, patch, patch), (3,))
    pairs = [_guarded(s, torch.int32 if len(s) == 1 else torch.float32) for s in shapes]
    out = _run_train(_dev(_train_batch(patch, names, sets)), 25, patch, out=tuple(v for _, v in pairs))
    torch.cuda.synchronize()
    got = _host(out)
    for i, n in enumerate(names):
        _assert_pair(got, i, expected(patch, n, 25, *sets[i]), n)
    for buf, view in pairs:
        raw = buf.cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
        assert not (view.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).any()
    images = [PC.fixture_image(3, 0), PC.fixture_image(4, 1)[:7, :5].copy()]
    psets = list(fixture_sets()[:2])
    b = _pack_images(images, psets)
    buf, view = _guarded((b["packed"].size,), torch.uint8)
    _photo(b, 0, out=view)
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    want = np.concatenate([PC.distort(im, p, q).reshape(-1) for im, (p, q) in zip(images, psets)])
    assert np.array_equal(raw[GUARD:-GUARD], want)


def test_both_entry_points_capture_into_a_graph_and_replay():
    patch = 16
    names = S.batch_names(patch, 5)
    sets = _sets_for(names)
    d = _dev(_train_batch(patch, names, sets))
    want = _host(_run_train(d, 25, patch))
    want_photo = ops.photometric_u8(d["packed"], d["offsets"][:2], d["sizes"][:2], d["params"][:2], d["perm"][:2], 2).cpu().numpy()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # (outputs and workspace come from the graph's own pool)
        out = _run_train(d, 25, patch)
        photo = ops.photometric_u8(d["packed"], d["offsets"][:2], d["sizes"][:2], d["params"][:2], d["perm"][:2], 2)
    for t in out:
        t.fill_(7)                                                   # stale contents: the replay must rewrite everything
    photo.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, w in zip(_host(out), want):
        assert np.array_equal(a.view(np.uint32), w.view(np.uint32))
    assert np.array_equal(photo.cpu().numpy(), want_photo) and want_photo.any()


# ---- SyntheticPairs(photometric_seed=...) -----------------------------------------------------------------------------------
def test_synthetic_pairs_training_task():
    """Two iterations give the same batches; the source side is the validation task's, the destination patch is not, and is
    the restatement's for the parameters the loader reports; a short train_head run through TrainableStage4 on one 64 x 64
    pair has a finite, falling loss."""
    hom = {"perspective": 0.1, "rotation": 10, "scale": 0.05}
    ims = S.images()
    labels = [S.make_labels("uniform", 600, im.shape[:2], 321 + i) for i, im in enumerate(ims)]

    def loader(photometric_seed):
        return SyntheticPairs(ims, labels, hom, 64, 0, 5, batch_pairs=2, device=DEV, photometric_seed=photometric_seed)

    train, val = loader(7), loader(None)
    first = [tuple(t.clone() for t in batch) for batch in train]
    second = [tuple(t.clone() for t in batch) for batch in train]
    plain = [tuple(t.clone() for t in batch) for batch in val]
    assert len(first) == len(second) == len(plain) == 2 and val.last_photometric is None and len(train.last_photometric) == 2
    rng, prng = random.Random(5), np.random.RandomState(7)
    for i in range(2):
        for a, b in zip(first[i], second[i]):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), i
        for k in (0, 2, 3, 4, 5):
            assert np.array_equal(_bits(first[i][k].cpu().numpy()), _bits(plain[i][k].cpu().numpy())), (i, k)
        assert not np.array_equal(first[i][1].cpu().numpy(), plain[i][1].cpu().numpy()), i
        geo = DU.sample_pair_geometry(ims[i].shape, hom, 64, rng, photometric_rng=prng)
        ph = train.last_photometric[i]
        assert np.array_equal(ph["params"], geo["photometric"]["params"]) and ph["perm"] == geo["photometric"]["perm"]
        warped = S.crop(S.warp_perspective_u8(PC.distort(ims[i], ph["params"], ph["perm"], blue_idx=2), geo["inv_h"]), geo["win_dst"], 64)
        assert np.array_equal(_bits(first[i][1][0].cpu().numpy()), _bits(S.norm255(warped).transpose(2, 0, 1))), i
        assert int(train.last_dst_max[i]) == int(warped.max())
    chunk = first[:1]
    assert chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(2))
    model.precision = "fp32"
    model = model.eval().to(DEV)
    stage = TrainableStage4.from_model(model)
    opt = torch.optim.Adam(stage.parameters(), lr=1e-3)
    losses = [train_utils.train_head(chunk, model, stage, opt, DEV, noise=False) for _ in range(6)]
    print("train_head on one distorted pair:", [round(v, 4) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
