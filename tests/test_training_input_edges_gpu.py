"""The training-input leg past one workgroup's stride: balf_synth_pairs and balf_detector_loss
(include/balf_hip.h) at the sizes where their loops take a second step -- more than 1024 workgroup maxima, more label rows
than the label kernel has threads, ties wider than one pass, more than 64 per-workgroup partials -- and at the edges of their
arithmetic: truncation, a zero denominator, landings on .5 and on the last row and column, the pole of the image warp, a
singular matrix, outputs that are only 4-byte aligned, patches below one store.  Pair synthesis is compared bit for bit with
pair_synth_common.pair_np; the loss is gated exactly as test_detector_loss_gpu.check_against gates it, against
detector_loss_common.restate64 within the fixture's tol_loss / tol_grad.  The cases and their CPU properties:
tests/training_input_common.py, tests/test_training_input_edges_host.py."""
import numpy as np
import pytest
import torch

from balf_amd import ops
from tests import detector_loss_common as D
from tests import pair_synth_common as S
from tests import training_input_common as T
from tests.test_detector_loss_gpu import bits_equal, check_against, run_all
from tests.test_guard_gpu import GUARD, PAT, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- A. balf_synth_pairs ---------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(call, out=None):
    d = {k: torch.from_numpy(v).to(DEV) for k, v in T.pack_call(call).items()}
    return ops.synth_pairs(d["packed"], d["offsets"], d["sizes"], d["inv_h"], d["win_src"], d["win_dst"], d["pts"],
                           d["pts_offsets"], call["top_k"], call["patch"], out=out)


def _host(out):
    return [t.cpu().numpy() for t in out]


def _assert_pair(got, i, want, what):
    """Pair i of a call's five host arrays against a (img_src, img_dst, heat_src, heat_dst, dst_max) tuple, bit for bit."""
    for k, (a, w) in enumerate(zip(got[:4], want[:4])):
        assert a[i].shape == w.shape and np.array_equal(_bits(a[i]), _bits(w)), (what, i, ("img_src", "img_dst", "heat_src", "heat_dst")[k])
    assert int(got[4][i]) == int(want[4]), (what, i, int(got[4][i]), int(want[4]))


def _assert_call(call, got=None):
    got = _host(_run(call)) if got is None else got
    p, patch = len(call["pairs"]), call["patch"]
    assert got[0].shape == got[1].shape == (p, 3, patch, patch) and got[2].shape == got[3].shape == (p, 1, patch, patch)
    for i, pair in enumerate(call["pairs"]):
        _assert_pair(got, i, T.expected_pair(call, i), pair["name"])
    return got


@pytest.mark.parametrize("patch", T.BIG_PATCHES)
def test_dst_max_over_1024_and_more_workgroup_maxima(patch):
    """nblk = 1024 exactly and 1033: the only byte above 100 is sampled by the last row, whose workgroups are the last of the
    pair; the second pair of the call has no such byte.  The image kernel runs more than 1024 workgroups in x."""
    call = T.big_patch_call(patch)
    got = _assert_call(call)
    assert int(got[4][0]) == T.BRIGHT and 0 < int(got[4][1]) <= T.DIM
    row, col, ch = T.bright_at(patch)
    assert got[1][0, ch, row, col] == 1.0 and np.count_nonzero(_bits(got[1][0]) != _bits(got[1][1])) == 1


@pytest.mark.parametrize("top_k", T.ROW_TOP_KS)
def test_more_label_rows_than_threads(top_k):
    """1023, 1024, 1025 and 5000 rows in one call, every row on a pixel of its own in the source window: the source heat map
    counts the kept rows."""
    call = T.many_rows_call(top_k)
    got = _assert_call(call)
    for i, n in enumerate(T.ROW_COUNTS):
        assert int(got[2][i].sum()) == (n if top_k == 0 or n <= top_k else top_k), (top_k, n)


def test_second_select_over_wide_ties():
    """All 5000 probs equal; 40 tied rows spread over 4563 indices, 17 of them inside the cut; -0.0 and +0.0 on either side
    of the cut, which compare equal; negative probs.  In plain terms: the source heat map is 1.0 at exactly the rows
    training_input_common.wide_tie_kept writes down."""
    call = T.wide_tie_call()
    got = _assert_call(call)
    kept = T.wide_tie_kept()
    for i, p in enumerate(call["pairs"]):
        want = np.zeros((T.ROWS_PATCH, T.ROWS_PATCH), np.float32)
        xy = p["pts"][kept[p["name"]], :2].astype(np.int64) - np.asarray(p["win_src"])[::-1]
        want[xy[:, 1], xy[:, 0]] = 1.0
        assert int(got[2][i].sum()) == T.TIE_TOP_K and np.array_equal(got[2][i, 0], want), p["name"]


@pytest.fixture(scope="module")
def edge_batch():
    """One call of the twelve edge pairs at patch 32, keep-all."""
    call = T.edge_call(T.EDGE_PATCH)
    return call, _host(_run(call))


@pytest.mark.parametrize("name", T.edge_names())
def test_edge_pair_equals_the_restatement(edge_batch, name):
    call, got = edge_batch
    i = T.edge_names().index(name)
    _assert_pair(got, i, T.expected_pair(call, i), name)
    assert got[2][i].any()                                                  # every pair has labels in its source window


def test_label_geometry_in_plain_terms(edge_batch):
    """Independent of the restatement: where the special rows of the label-geometry pairs must land."""
    call, got = edge_batch
    names, patch = T.edge_names(), T.EDGE_PATCH
    (ha, wa), _ = T.EDGE_SHAPES
    hs = got[2][names.index("trunc"), 0]                                    # window (0, 0): x, y in (-1, 0) -> column / row 0
    assert hs[3, 0] == hs[0, 4] == hs[0, 0] == 1.0
    p = call["pairs"][names.index("zn_zero")]
    hd = got[3][names.index("zn_zero"), 0]                                  # x = 8 -> zn = 0.5 -> column 16; x = 16 -> zn = 0: dropped
    assert hd[int(p["pts"][8, 1]) * 2, 16] == 1.0
    alone = dict(call, pairs=[dict(p, pts=p["pts"][16:17])])
    assert not _host(_run(alone))[3].any()
    p = call["pairs"][names.index("half")]
    hd = got[3][names.index("half"), 0]                                     # x + 2.5, y + 3.5: half to even
    for x, y in p["pts"][:36, :2].astype(np.int64):
        cx, cy = x - p["win_dst"][1], y - p["win_dst"][0]
        ex, ey = cx + 2 + (x % 2) * 1, cy + 3 + (1 - y % 2) * 1             # 2.5 -> 2, 3.5 -> 4; 3.5 -> 4, 4.5 -> 4
        if ex < patch and ey < patch:
            assert hd[ey, ex] == 1.0, (x, y)
    hd = got[3][names.index("on_max"), 0]                                   # the window ends on the last row and column
    assert hd[patch - 2, patch - 1] == hd[patch - 1, patch - 2] == hd[patch - 1, patch - 1] == 1.0


def test_pole_and_singular_in_plain_terms(edge_batch):
    """W == 0: the tap is pixel (0, 0) of the source; a saturated coordinate samples nothing.  det == 0: an all-zero
    destination patch and dst_max == 0, the heat maps still there, the neighbours as in a call of their own."""
    call, got = edge_batch
    names, patch = T.edge_names(), T.EDGE_PATCH
    corner = S.norm255(T.edge_images()[0][0, 0])
    col = T.POLE_COLUMN - call["pairs"][names.index("pole")]["win_dst"][1]
    d = got[1][names.index("pole")]
    assert np.array_equal(_bits(d[:, :, col]), _bits(np.repeat(corner[:, None], patch, axis=1)))
    for n in ("pole_neg", "pole_pos"):
        d = got[1][names.index(n)]
        assert np.array_equal(_bits(d[:, 0, col]), _bits(corner)) and not d[:, 1:, col].any()
    for n in T.SINGULAR:
        i = names.index(n)
        assert not got[1][i].any() and int(got[4][i]) == 0 and got[0][i].all() and got[2][i].any()
        for j in (i - 1, i + 1):
            one = _host(_run(T.single(call, j)))
            _assert_pair(got, j, [a[0] for a in one[:4]] + [one[4][0]], names[j])
            assert int(got[4][j]) > 0
    assert got[3][names.index("zero_row")].any()                            # y' = 0 / zn: row 0 of the image, not dropped


@pytest.mark.parametrize("which", range(4))
def test_outputs_four_bytes_off_alignment_take_the_scalar_stores(which):
    """patch = 32 would take the 16-byte stores; one float output in turn starts 4 bytes into its 16-byte aligned buffer.
    Same bits as the aligned call, nothing written outside."""
    call = dict(T.edge_call(T.EDGE_PATCH, top_k=25), pairs=T.edge_pairs(T.EDGE_PATCH)[:5])
    want = _run(call)
    assert all(t.data_ptr() % 16 == 0 for t in want[:4])
    bands, out = [], []
    for k, t in enumerate(want):
        g = Guarded(t.numel() * 4 + (4 if k == which else 0))
        lead = 4 if k == which else 0
        view = g.full[GUARD + lead:GUARD + lead + t.numel() * 4].view(t.dtype).view(t.shape)
        assert view.data_ptr() % 16 == lead and view.is_contiguous()
        bands.append(g)
        out.append(view)
    got = _run(call, out=tuple(out))
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in out]
    for k, (a, w, g) in enumerate(zip(got, want, bands)):
        assert g.intact() and bool((g.full[GUARD:GUARD + (4 if k == which else 0)] == PAT).all()), k
        assert bits_equal(a, w), k
    _assert_call(call, _host(got))


@pytest.mark.parametrize("patch", T.TINY_PATCHES)
def test_tiny_patches(patch):
    """patch = 1, 2, 3, 5: rows shorter than one store, a single quad per row, a ragged last quad."""
    got = _assert_call(T.edge_call(patch, top_k=25))
    assert got[1].any() and got[2].any()


def test_sixty_four_pairs_in_one_call():
    """The reference's call size: 64 pairs of patch 8 cycling the edge pairs, two of them with 1100 rows.  Every pair against
    the restatement; four of them (a singular one, the pole, a 1100-row pair, the last) against a call of their own."""
    call = T.many_pairs_call()
    got = _assert_call(call)
    for i in T.MANY_SPOT:
        one = _host(_run(T.single(call, i)))
        _assert_pair(got, i, [a[0] for a in one[:4]] + [one[4][0]], i)


# ---- B. balf_detector_loss -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return D.fixture()


def _restate(c):
    return D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"])


@pytest.mark.parametrize("masked", (True, False))
@pytest.mark.parametrize("hc,wc", T.LOSS_PLANES + T.LOSS_THIN)
def test_loss_with_one_wave_of_partials_and_more(fx, hc, wc, masked):
    """nblk = 63, 64, 65 and the one-pixel-thin planes of 66: B = 3, the last image fully masked in the masked run."""
    c = T.loss_case(hc, wc, masked)
    out = run_all(c)
    check_against(out, _restate(c), fx, f"{hc}x{wc} nblk {T.loss_nblk(hc, wc)} {'mask, noise' if masked else 'no mask, no noise'}")
    if masked:
        assert float(out.per_image[2]) == 0.0 and not out.dlogits[2].any()
    assert torch.isfinite(out.loss) and float(out.loss) > 0


@pytest.mark.parametrize("masked", (True, False))
def test_loss_on_the_workload_plane(fx, masked):
    """136 x 240 cells, 128 partials per image, B = 2, both images valid."""
    hc, wc = T.LOSS_WORKLOAD
    c = T.loss_case(hc, wc, masked, b=2, last_masked=False)
    out = run_all(c)
    check_against(out, _restate(c), fx, f"workload plane {'mask, noise' if masked else 'no mask, no noise'}")
    assert float(out.per_image.min()) > 0


@pytest.mark.parametrize("hc,wc", T.LOSS_PLANES)
def test_loss_partials_sum_in_a_fixed_order(hc, wc):
    """The same call twice: the same bits.  Image b of the batch run alone: the same per-image bits and labels (per_image does
    not carry the 1 / B of the gradient's scale, so nothing has to be undone for it)."""
    c = T.loss_case(hc, wc, True)
    abc, abc2 = run_all(c), run_all(c)
    for a, b in zip(abc, abc2):
        assert bits_equal(a, b)
    for b in range(3):
        alone = run_all({k: v[b:b + 1].contiguous() for k, v in c.items()})
        assert bits_equal(alone.per_image[0], abc.per_image[b]) and torch.equal(alone.labels[0], abc.labels[b]), b
        assert bits_equal(alone.loss, alone.per_image[0])
        # the gradient of a batch of one is B times the batch's: within one float32 rounding of each other
        assert torch.allclose(alone.dlogits[0] / 3.0, abc.dlogits[b], rtol=2.0 ** -22, atol=0.0), b
    assert float(abc.per_image[0]) > 0 and float(abc.per_image[2]) == 0.0


def test_loss_when_every_valid_cell_lies_past_the_first_wave_of_partials(fx):
    """Image 0's valid cells are the 126 of workgroup 64: partials 0..63 hold 256 * fl32(1e-6) and 0.0 only."""
    c = T.late_cells_case()
    out = run_all(c)
    r = _restate(c)
    check_against(out, r, fx, "late cells")
    assert float(out.per_image[0]) > 1.0 and bool(torch.isfinite(out.per_image).all())
    g = out.dlogits[0].reshape(65, -1)
    assert not g[:, :T.LATE_FIRST_CELL].any() and bool(g[:, T.LATE_FIRST_CELL:].all())
