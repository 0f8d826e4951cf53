"""balf_synth_pairs on the GPU (include/balf_hip.h; ops.synth_pairs, datasets/synthetic_pairs.SyntheticPairs) against
tests/golden/pair_synth.npz -- heat maps, source patches, byte / 255 and the pair geometry, recorded from the reference's own
functions by tests/golden/make_pair_synth_golden.py -- and against tests/pair_synth_common.py's integer restatement of the
8-bit warp (destination patch, dst_max).  Every comparison is EXACT: the outputs are integer-derived.  Only the fixture is
read here, never the reference tree."""
import random

import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets import dataset_utils as DU
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.utils import synth, train_utils
from tests import pair_synth_common as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return S.fixture()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _run(patch, names, labels, top_k, out=None):
    d = _dev(S.pack_batch(patch, names, labels))
    return ops.synth_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"],
                           d["pts_offsets"], top_k, patch, out=out)


def _labels(g):
    return {str(n): g[f"labels.{n}"] for n in g["meta.cases"]}


def _host(out):
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("patch", S.PATCHES)
@pytest.mark.parametrize("p", S.BATCHES)
@pytest.mark.parametrize("top_k", S.TOP_KS)
def test_batch_against_fixture_and_restatement(g, patch, p, top_k):
    """P pairs of both image sizes in one call.  Against the fixture: both heat maps, the source patch where recorded, byte /
    255.  Against the restatement: the destination patch and dst_max (and the source patch everywhere).  And the batch equals
    P one-pair calls."""
    names = S.batch_names(patch, p)
    labels = _labels(g)
    img_s, img_d, heat_s, heat_d, dst_max = _host(_run(patch, names, labels, top_k))
    assert img_s.shape == img_d.shape == (p, 3, patch, patch) and heat_s.shape == heat_d.shape == (p, 1, patch, patch)
    table = g["norm255"]
    for i, n in enumerate(names):
        key = f"p{patch}.{n}.k{top_k}"
        assert np.array_equal(heat_s[i, 0], g[f"{key}.heat_src"].astype(np.float32)), (key, i)
        assert np.array_equal(heat_d[i, 0], g[f"{key}.heat_dst"].astype(np.float32)), (key, i)
        if f"p{patch}.{n}.img_src" in g:
            assert np.array_equal(_bits(img_s[i]), _bits(g[f"p{patch}.{n}.img_src"])), (key, i)
        e = S.expected(patch, n, top_k)
        assert np.array_equal(_bits(img_s[i]), _bits(e[0])), (key, i)
        assert np.array_equal(_bits(img_d[i]), _bits(e[1])), (key, i, np.abs(img_d[i] - e[1]).max() * 255)
        assert int(dst_max[i]) == e[4], (key, i)
        assert np.isin(_bits(img_d[i]), _bits(table)).all()                           # every value is a byte / 255
    if p == max(S.BATCHES):
        assert {"outside", "last_col", "rot25_half", "mild_tie"} <= set(names)
        for i, n in enumerate(names):                                                 # the batch equals P one-pair calls
            one = _host(_run(patch, [n], labels, top_k))
            for a, b in zip(one[:4], (img_s, img_d, heat_s, heat_d)):
                assert np.array_equal(_bits(a[0]), _bits(b[i])), (n, i)
            assert int(one[4][0]) == int(dst_max[i])


def test_identity_translation_and_outside_in_plain_terms(g):
    """Independent of the restatement: identity with coinciding windows copies the source patch; an integer translation gives a
    shifted copy, zero where the taps leave the source; a window sampling outside gives zeros and dst_max == 0."""
    patch = 32
    ims, cs, labels = S.images(), S.cases(patch), _labels(g)
    names = ["identity_tl", "identity_br", "shift_int", "outside"]
    img_s, img_d, _, heat_d, dst_max = _host(_run(patch, names, labels, 0))
    assert np.array_equal(_bits(img_d[0]), _bits(img_s[0])) and np.array_equal(_bits(img_d[1]), _bits(img_s[1]))
    assert int(dst_max[0]) == int(S.crop(ims[0], (0, 0), patch).max())
    c = cs["shift_int"]                                              # dst(x, y) = src(x - 20, y + 7)
    full = np.zeros_like(ims[0])
    full[:-7, 20:] = ims[0][7:, :-20]
    want = S.norm255(S.crop(full, c["win_dst"], patch)).transpose(2, 0, 1)
    assert np.array_equal(_bits(img_d[2]), _bits(want))
    assert not img_d[3].any() and not heat_d[3].any() and int(dst_max[3]) == 0


def test_second_call_into_the_same_buffers_leaves_nothing_stale(g):
    """Same output tensors and workspace, different inputs: the heat maps are re-zeroed, dst_max rewritten."""
    patch, labels = 64, _labels(g)
    first = ["mild", "dups", "rot25_half"]
    second = ["outside", "no_labels", "one_label"]
    out = _run(patch, first, labels, 0)
    assert out[2].sum() > 0 and out[3].sum() > 0
    ptrs = [t.data_ptr() for t in out]
    out2 = _run(patch, second, labels, 25, out=out)
    assert [t.data_ptr() for t in out2] == ptrs
    got = _host(out2)
    for i, n in enumerate(second):
        e = S.expected(patch, n, 25)
        for a, b in zip(got[:4], e[:4]):
            assert np.array_equal(_bits(a[i]), _bits(b)), n
        assert int(got[4][i]) == e[4]


def test_windows_that_leave_the_image_are_handled_on_the_device(g):
    """The windows live on the device, so the host cannot refuse them: reads are clamped, dst_max = -1; the neighbouring
    pair of the batch is untouched.  An image that does not lie inside the packed buffer gives zeros."""
    patch, labels = 32, _labels(g)
    names = ["mild", "mild", "mild", "identity_tl"]
    b = S.pack_batch(patch, names, labels)
    b["win_src"][0] = (-5, 120)                                      # leaves the 96 x 128 image on two sides
    b["win_dst"][1] = (90, 3)
    b["offsets"][2] = b["packed"].size - 100                         # the image would end outside the buffer
    d = _dev(b)
    out = _host(ops.synth_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"],
                                d["pts_offsets"], 0, patch))
    assert list(out[4][:3]) == [-1, -1, -1]
    im = S.images()[0]
    ys, xs = np.clip(np.arange(-5, -5 + patch), 0, 95), np.clip(np.arange(120, 120 + patch), 0, 127)
    assert np.array_equal(_bits(out[0][0]), _bits(S.norm255(im[np.ix_(ys, xs)]).transpose(2, 0, 1)))
    assert all(not out[k][2].any() for k in range(4))
    e = S.expected(patch, "identity_tl", 0)
    for a, w in zip(out[:4], e[:4]):
        assert np.array_equal(_bits(a[3]), _bits(w))
    assert int(out[4][3]) == e[4]
    e = S.expected(patch, "mild", 0)
    assert np.array_equal(_bits(out[1][0]), _bits(e[1])) and np.array_equal(_bits(out[0][1]), _bits(e[0]))


def test_odd_patch_takes_the_scalar_store_path(g):
    """patch = 30 is no multiple of the four pixels a thread writes at once."""
    patch, labels = 30, _labels(g)
    names = ["mild", "rot25_half"]
    cs = S.cases(32)
    ims = S.images()
    b = S.pack_batch(32, names, labels)
    d = _dev(b)
    out = _host(ops.synth_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"],
                                d["pts_offsets"], 25, patch))
    for i, n in enumerate(names):
        c = cs[n]
        e = S.pair_np(ims[c["image"]], labels[n], 25, c["inv_h"], c["win_src"], c["win_dst"], patch)
        for a, w in zip(out[:4], e[:4]):
            assert np.array_equal(_bits(a[i]), _bits(w)), n
        assert int(out[4][i]) == e[4]


def test_graph_capture_and_two_replays_give_the_same_bits(g):
    patch, labels = 64, _labels(g)
    names = S.batch_names(patch, 5)
    d = _dev(S.pack_batch(patch, names, labels))
    args = (d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"], d["pts_offsets"], 25, patch)
    want = _host(ops.synth_pairs(*args))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # (outputs and workspace come from the graph's own pool)
        out = ops.synth_pairs(*args)
    for _ in range(2):
        for t in out:
            t.fill_(7)                                               # stale contents: the replay must rewrite everything
        graph.replay()
        torch.cuda.synchronize()
        for a, w in zip(_host(out), want):
            assert np.array_equal(a.view(np.uint32), w.view(np.uint32))


def test_synthetic_pairs_feeds_check_val_repeatability(g):
    """End to end on 5 pairs of 128 x 128 patches: the ten values from SyntheticPairs equal those from feeding the same function
    the restatement's pairs (same geometry draws); both paths share the forward, so the equality is exact.  Also: the loader's
    tuples have the reference's shapes, and its homographies are sample_pair_geometry's."""
    hom = {"perspective": 0.2, "rotation": 25, "scale": 0.1}
    patch, top_k, seed = 128, 30, 11
    ims, labels = [], []
    for i in range(5):
        h, w = ((200, 264), (192, 256))[i % 2]
        gray = synth.synthetic_gray_u8(h, w, 40 + i)
        ims.append(np.ascontiguousarray(np.stack([gray, gray, gray], axis=2)))
        labels.append(S.make_labels("uniform", 60, (h, w), 300 + i))
    loader = SyntheticPairs(ims, labels, hom, patch, top_k, seed, batch_pairs=3, device=DEV)
    assert len(loader) == 5
    rng = random.Random(seed)
    want = []
    for im, pts in zip(ims, labels):
        geo = DU.sample_pair_geometry(im.shape, hom, patch, rng)
        e = S.pair_np(im, pts, top_k, geo["inv_h"], geo["win_src"], geo["win_dst"], patch)
        want.append(tuple(torch.from_numpy(np.ascontiguousarray(a))[None] for a in e[:4]) +
                    (torch.from_numpy(geo["h_src_2_dst"])[None], torch.from_numpy(geo["h_dst_2_src"])[None]))
    got = list(loader)
    assert len(got) == 5 and loader.last_dst_max.shape == (2,) and int(loader.last_dst_max.min()) > 0
    for a, b in zip(got, want):
        assert len(a) == 6
        for x, y in zip(a, b):
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == tuple(y.shape)
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.numpy()))
    assert sum(float(a[2].sum()) for a in got) > 0 and sum(float(a[3].sum()) for a in got) > 0
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(3))
    model = model.eval().to(DEV)
    ten_gpu = train_utils.check_val_repeatability(loader, model, DEV, None, 0, nms_size=15, num_points=25)
    ten_np = train_utils.check_val_repeatability(want, model, DEV, None, 0, nms_size=15, num_points=25)
    assert len(ten_gpu) == 10
    assert np.array_equal(np.asarray(ten_gpu, np.float64).view(np.uint64), np.asarray(ten_np, np.float64).view(np.uint64))
