"""NMS score maps on the GPU (balf_nms_score_map): both protocols against the NumPy oracle of tests/nms_map_common.py,
which tests/test_nms_map_host.py proves equal to the fixture recorded from the reference.  Equality is exact everywhere: the
outputs are copies of input scores and the selection is discrete, so there is no tolerance.

Every call through the C ABI (``abi``) runs on buffers of exactly the documented / queried sizes between patterned guard bands
(tests/test_guard_gpu.py: Guarded), with ``out`` pre-filled with NaN and the workspace with the guard pattern: a write outside a
buffer, an element of ``out`` that nobody wrote, a -0.0 and a read of a workspace slot that the call did not initialise all fail
the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd.benchmark_test import repeatability_tools
from balf_amd.utils import train_utils
from tests import nms_map_common as M
from tests.test_guard_gpu import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONF = M.CONF


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def abi(scores, protocol, conf=CONF, dist=0, size=None, iou=None, k=-1):
    """balf_nms_score_map on ``scores`` [B,H,W] -> (maps [B,H,W], counts [B]) as NumPy."""
    l = _lib.lib()
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    b, h, w = scores.shape
    code = ops.NMS_MAP_PROTOCOLS[protocol]
    prob = Guarded(b * h * w * 4, fill=0)
    prob.view(torch.float32, (b, h, w))[:] = torch.from_numpy(scores).to(DEV)
    out, count = Guarded(b * h * w * 4), Guarded(b * 4)
    out.view(torch.float32, (b, h, w))[:] = float("nan")
    n = C.c_size_t(0)
    assert l.balf_nms_score_map_sizes(b, h, w, code, C.byref(n)) == 0
    ws = Guarded(n.value)
    radius, rows = 0, None
    if protocol == "box":
        radius, table = ops.box_footprint(size, iou)
        rows = (C.c_uint64 * len(table))(*table)
    args = (prob.ptr, b, h, w, code, conf, dist, rows, radius, k, out.ptr, count.ptr, ws.ptr)
    assert l.balf_nms_score_map(*args, ws.n - 1, _stream()) == -3          # one byte short of the queried size: refused
    rc = l.balf_nms_score_map(*args, ws.n, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for name, g in (("prob", prob), ("out", out), ("count", count), ("workspace", ws)):
        assert g.intact(), f"balf_nms_score_map wrote outside {name} ({protocol}, {b} x {h}x{w})"
    assert bool((prob.view(torch.float32, (b, h, w)).cpu() == torch.from_numpy(scores)).all())      # the input is read-only
    return out.view(torch.float32, (b, h, w)).cpu().numpy(), count.view(torch.int32, (b,)).cpu().numpy()


def oracle(scores, protocol, conf=CONF, dist=0, size=None, iou=None, k=-1):
    fp = M.box_footprint_direct(size, iou) if protocol == "box" else M.square_footprint(dist)
    res = [M.sweep(s, conf, fp, k) for s in scores]
    return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], dtype=np.int32)


def check(scores, protocol, **kw):
    """C ABI against the oracle on a batch; -> (maps, counts)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    got, cnt = abi(scores, protocol, **kw)
    want, want_cnt = oracle(scores, protocol, **kw)
    assert not np.isnan(got).any()
    assert M.same_map(got, want), (protocol, kw, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8])
    assert np.array_equal(cnt, want_cnt), (protocol, kw, cnt, want_cnt)
    return got, cnt


def both(scores, radius3=True):
    """Both protocols at a footprint radius of 3 (the reference's default box, dist_thresh 3) or 16."""
    if radius3:
        check(scores, "box", size=4, iou=0.1)
        check(scores, "greedy", dist=3)
    else:
        check(scores, "box", size=17, iou=0.05)
        check(scores, "greedy", dist=16)


def random_scores(seed, b, h, w, tied=False):
    """Scores in [0, 0.05): about 70 % of them candidates; ``tied``: only 24 distinct values, so ties everywhere."""
    v = np.random.RandomState(seed).random_sample((b, h, w)).astype(np.float32)
    if tied:
        v = np.floor(v * 24) / 24
    return (v * np.float32(0.05)).astype(np.float32)


# ---- the fixture recorded from the reference, through every door ------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_cases():
    return M.fixture_cases(M.fixture())


@pytest.mark.parametrize("door", ["abi", "ops", "named"])
def test_fixture_cases(fixture_cases, door):
    for case, score, label, want, call in fixture_cases:
        if door == "abi":
            kw = dict(size=call[1], iou=call[2], k=call[3]) if call[0] == "box" else dict(dist=call[1])
            got, cnt = abi(score[None], call[0], **kw)
            got = got[0]
            assert cnt[0] == np.count_nonzero(want), (case, label)
        elif door == "ops":
            t = torch.from_numpy(score).to(DEV)[None]
            if call[0] == "box":
                got, cnt = ops.nms_score_map(t, "box", conf_thresh=CONF, size=call[1], iou=call[2], keep_top_k=call[3])
            else:
                got, cnt = ops.nms_score_map(t, "greedy", conf_thresh=CONF, dist_thresh=call[1])
            assert got.device == t.device and got.dtype == torch.float32 and tuple(got.shape) == (1,) + score.shape
            assert int(cnt[0]) == np.count_nonzero(want), (case, label)
            got = got[0].cpu().numpy()
        elif call[0] == "box":
            t = torch.from_numpy(score).to(DEV)[None]
            got = repeatability_tools.box_nms(t, call[1], call[2], CONF, call[3])
            assert got.device == t.device and tuple(got.shape) == (1,) + score.shape
            assert torch.equal(got, repeatability_tools.box_nms_batch(t, call[1], call[2], CONF, call[3]))
            got = got[0].cpu().numpy()
        else:
            got = repeatability_tools.apply_nms_fast(score, call[1], CONF)
            other = repeatability_tools.get_nms_score_map_from_score_map(score, CONF, call[1])
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and M.same_map(got, other)
        assert M.same_map(got, want), (door, case, label)


# ---- tile geometry: 64 x 32 tiles, a halo of the footprint radius -------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("h", [1, 31, 32, 33, 65])
def test_tile_geometry(h, w):
    scores = np.concatenate([random_scores(h * 1000 + w, 1, h, w), random_scores(h * 1000 + w + 1, 1, h, w, tied=True)])
    both(scores)


def _boundary_images(radius, victim_first):
    """One image per direction (dy, dx): a strong point on the edge of the central tile of a 3 x 3 tile map and a weaker one
    ``radius`` further in that direction, inside the neighbour tile (``victim_first``: the strong one is the outer one), and a
    third, weakest, one step beyond."""
    dirs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    imgs = np.zeros((len(dirs), 96, 192), dtype=np.float32)
    pairs = []
    for i, (dy, dx) in enumerate(dirs):
        ay = 32 if dy < 0 else (63 if dy > 0 else 48)
        ax = 64 if dx < 0 else (127 if dx > 0 else 96)
        by, bx = ay + radius * dy, ax + radius * dx
        imgs[i, ay, ax], imgs[i, by, bx] = (0.5, 0.9) if victim_first else (0.9, 0.5)
        imgs[i, by + dy, bx + dx] = 0.1
        pairs.append(((ay, ax), (by, bx)))
    return imgs, pairs


@pytest.mark.parametrize("victim_first", [False, True])
@pytest.mark.parametrize("radius", [3, 16])
def test_suppressor_across_every_side_and_corner_of_a_tile(radius, victim_first):
    imgs, pairs = _boundary_images(radius, victim_first)
    # the box footprints hold the whole square here: IoU(3, 3) of two 4 x 4 boxes is 1 / 31, IoU(16, 16) of two 17 x 17 ones 1 / 577
    for protocol, kw in (("box", dict(size=radius + 1, iou=0.001)), ("greedy", dict(dist=radius))):
        got, cnt = check(imgs, protocol, **kw)
        for i, (a, b) in enumerate(pairs):
            strong, weak = (b, a) if victim_first else (a, b)
            assert got[i][strong] == np.float32(0.9) and got[i][weak] == 0.0, (protocol, i)


def test_batch_of_different_images_one_empty_one_single():
    scores = random_scores(5, 3, 45, 100)
    scores[1] = np.float32(0.01)                               # no candidate at all
    scores[2] = 0.0
    scores[2, 44, 99] = 0.3                                     # a single one, in the last pixel
    for protocol, kw in (("box", dict(size=4, iou=0.1)), ("greedy", dict(dist=3))):
        got, cnt = check(scores, protocol, **kw)
        assert cnt[0] > 10 and cnt[1] == 0 and cnt[2] == 1 and got[2, 44, 99] == np.float32(0.3)
        assert not got[1].any()


def test_threshold_edge():
    conf = np.float32(CONF)
    scores = np.zeros((1, 3, 80), dtype=np.float32)
    scores[0, 1, 5] = conf                                      # >= : a candidate
    scores[0, 1, 45] = np.nextafter(conf, np.float32(0))        # the float just below: not one
    for protocol, kw in (("box", dict(size=4, iou=0.1)), ("greedy", dict(dist=4))):
        got, cnt = check(scores, protocol, **kw)
        assert cnt[0] == 1 and got[0, 1, 5] == conf and np.count_nonzero(got) == 1


# ---- many rounds: past the enqueued ones, the per-image tail kernel -----------------------------------------------------------------
def test_many_rounds_ramps_and_plateau():
    ramp = lambda h, w: (0.02 + np.arange(h * w, dtype=np.float32) * np.float32(1e-5)).reshape(1, h, w)      # noqa: E731
    for scores in (ramp(8, 200), ramp(40, 40), np.full((1, 33, 70), 0.5, dtype=np.float32)):      # the plateau: the tie rule alone
        both(scores)
    both(np.concatenate([ramp(40, 40), ramp(40, 40)[:, ::-1, ::-1], random_scores(9, 1, 40, 40)]), radius3=False)


# ---- keep_top_k ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [False, True])
def test_keep_top_k(tied):
    scores = random_scores(21, 2, 50, 90, tied=tied)
    for protocol, kw in (("box", dict(size=4, iou=0.1)), ("greedy", dict(dist=2))):
        _, full = check(scores, protocol, **kw)
        assert full.min() > 20
        for k in (1, 5, int(full[0]), int(full[0]) - 1, int(full.max()) + 7, 50 * 90, 50 * 90 + 1):
            got, cnt = check(scores, protocol, k=k, **kw)
            assert np.array_equal(cnt, np.minimum(full, k))
    if tied:                                                    # the cut falls inside a run of equal scores: the lower raster index stays
        got, _ = check(scores, "box", size=4, iou=0.1, k=5)
        kept = np.sort(got[0][got[0] > 0])
        full_map, _ = oracle(scores[:1], "box", size=4, iou=0.1)
        assert np.count_nonzero(full_map[0] == kept[0]) > np.count_nonzero(got[0] == kept[0])


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_box_protocol_replays_from_a_graph():
    inputs = [torch.from_numpy(random_scores(30 + i, 2, 70, 150, tied=(i == 1))).to(DEV) for i in range(3)]
    run = lambda x: ops.nms_score_map(x, "box", conf_thresh=CONF, size=4, iou=0.1, keep_top_k=40)      # noqa: E731
    static = inputs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up: LDS attributes, the workspace of this stream
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # (balf_nms_score_map enqueues every launch on the one stream it is given, so the captured work is a single chain by
    # construction; nothing here asserts the graph's shape)
    with torch.cuda.graph(graph):
        outs = run(static)
    for x in (inputs[1], inputs[2]):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        want = run(x)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
        ref, ref_cnt = oracle(x.cpu().numpy(), "box", size=4, iou=0.1, k=40)
        assert M.same_map(outs[0].cpu().numpy(), ref) and np.array_equal(outs[1].cpu().numpy(), ref_cnt)


# ---- the reference-named functions --------------------------------------------------------------------------------------------------
def test_prob_to_score_maps_tensor_batch_is_apply_nms_fast_per_image():
    prob = torch.from_numpy(random_scores(40, 3, 40, 72)).to(DEV)
    got = train_utils.prob_to_score_maps_tensor_batch(prob, 4)
    assert tuple(got.shape) == (3, 1, 40, 72) and got.dtype == torch.float32 and got.device == prob.device
    for i in range(3):
        one = repeatability_tools.apply_nms_fast(prob[i].cpu().numpy(), 4)
        assert M.same_map(got[i, 0].cpu().numpy(), one)
        assert M.same_map(one, M.greedy_oracle(prob[i].cpu().numpy(), 4)[0])


def _val_points_rows(score, num_points):
    """The source and the destination rows of balf_val_points' greedy leg (dist_thresh 4) for ``score`` paired with itself under the
    identity homography, as lists of (x, y, score)."""
    t = torch.from_numpy(score).to(DEV)[None]
    eye = torch.eye(3, dtype=torch.float64, device=DEV)[None]
    src, dst, count = ops.val_points(t, t, eye, 4, num_points, "greedy", CONF)
    return [[(int(round(x)), int(round(y)), np.float32(s)) for x, y, _, s in rows[0, :int(count[0, side])].cpu().numpy()]
            for side, rows in enumerate((src, dst))]


def test_score_map_against_the_nms_map_inside_val_points_greedy_leg():
    """balf_val_points builds the same NMS map internally (its greedy leg), masks it with the pair's common region -- under the
    identity homography the image without a border of 15 pixels -- and returns the ``num_points`` best of what is left.  It does not
    expose the map, so this is a check of the two maps THROUGH that selection, not an equality of maps:
      * every row it returns with a positive score is a survivor of get_nms_score_map_from_score_map's map, at its score (a
        survivor that this map lacks would fail here);
      * every survivor of this map that lies at least 20 pixels inside the image and scores above the weakest returned row is
        among the rows (a survivor that val_points' map lacks, or one that this map has in excess, would fail here).
    On the fixture inputs (40 x 72 and 33 x 130: a common region of a few rows) with 5 points, and on a 160 x 240 map with 300
    points, where the region holds about 700 survivors and the cut falls inside it."""
    fx = M.fixture()
    cases = [(case, fx[f"{case}.score"], 5) for case in M.CASES] + [("160x240", random_scores(77, 1, 160, 240)[0], 300)]
    for case, score, k in cases:
        nms = repeatability_tools.get_nms_score_map_from_score_map(score, CONF, 4)
        t = torch.from_numpy(score).to(DEV)[None]
        assert M.same_map(nms, ops.nms_score_map(t, "greedy", conf_thresh=CONF, dist_thresh=4)[0][0].cpu().numpy())
        if case in M.CASES:
            assert M.same_map(nms, fx[f"{case}.greedy_d4"])
        h, w = score.shape
        for rows in _val_points_rows(score, k):
            positive = [(x, y, s) for x, y, s in rows if s > 0]
            for x, y, s in positive:
                assert nms[y, x] == s, (case, x, y, s)
            if case == "160x240":
                assert len(positive) == k                        # the region holds more survivors than num_points
                weakest = min(s for _, _, s in positive)
                inner = np.zeros_like(nms, dtype=bool)
                inner[20:h - 20, 20:w - 20] = True
                must = {(int(x), int(y)) for y, x in np.argwhere(inner & (nms > weakest))}
                assert len(must) > 100 and must <= {(x, y) for x, y, _ in positive}, (case, len(must))
