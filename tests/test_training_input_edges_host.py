"""The CPU half of the training-input edges (the GPU half is tests/test_training_input_edges_gpu.py): every
property of the inputs that a GPU case relies on, asserted from NumPy alone, and the general packer against
pair_synth_common.pack_batch byte for byte.  The restatements used as references there are pinned to the recorded goldens by
test_pair_synth_host.py and test_detector_loss_host.py."""
import numpy as np
import pytest
import torch

from tests import detector_loss_common as D
from tests import pair_synth_common as S
from tests import training_input_common as T


# ---- the packer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", S.PATCHES)
@pytest.mark.parametrize("p", S.BATCHES)
def test_general_packer_reproduces_pack_batch(patch, p):
    g = S.fixture()
    labels = {str(n): g[f"labels.{n}"] for n in g["meta.cases"]}
    names = S.batch_names(patch, p)
    want = S.pack_batch(patch, names, labels)
    cs = S.cases(patch)
    got = T.pack_pairs(S.images(), [dict(image=cs[n]["image"], inv_h=cs[n]["inv_h"], win_src=cs[n]["win_src"],
                                         win_dst=cs[n]["win_dst"], pts=labels[n]) for n in names])
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


# ---- A. balf_synth_pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", T.BIG_PATCHES)
def test_bright_byte_is_sampled_by_the_last_row_only(patch):
    """... and by a workgroup past the first 1024 of the blk_max loop when patch = 1028; nblk is 1024 exactly and 1033."""
    assert T.image_blocks(patch) == T.BIG_NBLK[patch]
    call = T.big_patch_call(patch)
    bright, dim = call["images"]
    row, col, ch = T.bright_at(patch)
    assert bright.shape == (patch, patch, 3) and int(dim.max()) <= T.DIM and int(bright[row, col, ch]) == T.BRIGHT
    rest = bright.copy()
    rest[row, col, ch] = 0
    assert int(rest.max()) <= T.DIM and np.array_equal(np.delete(bright.reshape(-1), (row * patch + col) * 3 + ch),
                                                       np.delete(dim.reshape(-1), (row * patch + col) * 3 + ch))
    for p in call["pairs"]:
        assert p["win_dst"] == (0, 0) and np.array_equal(p["inv_h"], np.eye(3))
    ys, xs = np.mgrid[0:patch, 0:patch]
    sx, sy, fx, fy = S.source_q5(S.invert3(np.eye(3)), ys, xs)
    assert not fx.any() and not fy.any()                              # one tap of weight 32768 per pixel: (sy, sx)
    hit = (sy == row) & (sx == col)
    assert hit.sum() == 1 and set(np.nonzero(hit)[0]) == {patch - 1}
    qpr = (patch + T.IMG_PX - 1) // T.IMG_PX
    block = ((patch - 1) * qpr + col // T.IMG_PX) // T.IMG_THREADS
    assert block == T.BIG_NBLK[patch] - 1 and (block >= T.LBL_THREADS) == (patch == 1028)


def test_row_counts_cross_the_label_threads():
    assert T.ROW_COUNTS == (1023, 1024, 1025, 5000) and T.LBL_THREADS == 1024
    for n in T.ROW_COUNTS:
        assert {0, 1, n - 1, n, n + 1, n // 2} <= set(T.ROW_TOP_KS)
    call = T.many_rows_call(0)
    b = T.pack_call(call)
    assert b["pts_offsets"].tolist() == [0, 1023, 2047, 3072, 8072] and len(b["pts"]) == 8072
    for p in call["pairs"]:
        n = len(p["pts"])
        pix = p["pts"][:, :2].astype(np.int64) - np.asarray(p["win_src"])[::-1]
        assert (pix >= 0).all() and (pix < T.ROWS_PATCH).all()
        assert len(np.unique(pix[:, 1] * T.ROWS_PATCH + pix[:, 0])) == n            # one pixel of the source window per row
        assert len(np.unique(p["pts"][:, 2])) == n                                  # no ties: the first select decides alone
        h, w = call["images"][p["image"]].shape[:2]
        for win in (p["win_src"], p["win_dst"]):
            assert 0 <= win[0] <= h - T.ROWS_PATCH and 0 <= win[1] <= w - T.ROWS_PATCH


def test_wide_ties_straddle_the_cut():
    call, kept = T.wide_tie_call(), T.wide_tie_kept()
    assert call["top_k"] == T.TIE_TOP_K == 1500
    pairs = {p["name"]: p for p in call["pairs"]}
    assert set(pairs) == set(kept)
    for name, p in pairs.items():
        assert len(kept[name]) == T.TIE_TOP_K < len(p["pts"])
        assert np.array_equal(S.select_k_best(p["pts"], T.TIE_TOP_K), kept[name]), name
    assert np.array_equal(kept["all_equal"], np.arange(1500)) and len(np.unique(pairs["all_equal"]["pts"][:, 2])) == 1
    # the spread tie: 40 rows of one prob, 1483 rows above it, 17 of the group kept and 23 not, both parts wider than the
    # 1024 rows one pass of the label kernel's threads covers
    probs = pairs["spread_tie"]["pts"][:, 2]
    group = np.flatnonzero(probs == probs[T.TIE_GROUP[0]])
    assert np.array_equal(group, T.TIE_GROUP) and len(group) == 40 and (probs > probs[group[0]]).sum() == T.TIE_ABOVE
    inside = np.isin(group, kept["spread_tie"])
    assert inside[:17].all() and not inside[17:].any()
    assert group[16] - group[0] > T.LBL_THREADS and group[-1] - group[17] > T.LBL_THREADS and group[-1] - group[0] > 4 * T.LBL_THREADS
    assert len(np.unique(np.delete(probs, group))) == 5000 - 40
    # the zeros: ten of each sign, the lower indices -0.0 in one pair and +0.0 in the other, 1490 rows above them
    for name, first_negative in (("zeros_neg_first", True), ("zeros_pos_first", False)):
        probs = pairs[name]["pts"][:, 2]
        zeros = np.flatnonzero(probs == 0.0)
        assert len(zeros) == 20 and (probs > 0).sum() == 1490 and (probs < 0).sum() == 1490
        assert np.signbit(probs[zeros[:10]]).all() == first_negative and np.signbit(probs[zeros[10:]]).all() != first_negative
        assert np.signbit(probs[zeros[:10]]).any() == first_negative and np.signbit(probs[zeros[10:]]).any() != first_negative
        assert np.isin(zeros[:10], kept[name]).all() and not np.isin(zeros[10:], kept[name]).any()
    probs = pairs["negative"]["pts"][:, 2]
    assert (probs < 0).all() and len(np.unique(probs)) == 4000


def _pair(patch, name):
    return {p["name"]: p for p in T.edge_pairs(patch)}[name]


@pytest.mark.parametrize("patch", (T.EDGE_PATCH, T.MANY_PATCH) + T.TINY_PATCHES)
def test_edge_windows_lie_inside_their_images(patch):
    assert T.edge_names() == [p["name"] for p in T.edge_pairs(patch)]
    for p in T.edge_pairs(patch):
        h, w = T.EDGE_SHAPES[p["image"]]
        for win in (p["win_src"], p["win_dst"]):
            assert 0 <= win[0] <= h - patch and 0 <= win[1] <= w - patch, (p["name"], win)
        assert p["pts"].dtype == np.float32 and len(p["pts"]) >= 30
    assert all(im.min() > 0 for im in T.edge_images())                  # a tap inside an image is never 0


def test_label_geometry_properties():
    patch = T.EDGE_PATCH
    (ha, wa), (hb, wb) = T.EDGE_SHAPES
    # truncation toward zero: x, y in (-1, 0) land on column / row 0 and are kept; -1.0 and below, w and h are dropped
    p = _pair(patch, "trunc")
    xy = p["pts"][:11, :2]
    assert ((xy > -1) & (xy < 0)).any(axis=1).sum() == 3
    ints = xy.astype(np.int64)
    assert ints[:3].tolist() == [[0, 3], [4, 0], [0, 0]] and ints[3:6].tolist() == [[-1, 5], [5, -1], [-1, 2]]
    assert ints[6:10].tolist() == [[wa - 1, 2], [wa, 2], [2, ha - 1], [2, ha]]
    hs, _ = S.heatmaps(p["pts"][:11], 0, (ha, wa), p["inv_h"])
    assert hs[3, 0] == hs[0, 4] == hs[0, 0] == hs[2, wa - 1] == hs[ha - 1, 2] == hs[1, 1] == 1.0 and hs.sum() == 6.0
    # zn exactly 0 in float32, for the row with x = 16 and no other
    p = _pair(patch, "zn_zero")
    hm = p["inv_h"].astype(np.float32).reshape(9)
    assert float(hm[6]) == -1.0 / 16.0
    xi = p["pts"][:22, :2].astype(np.int64).astype(np.float32)
    zn = (hm[6] * xi[:, 0] + hm[7] * xi[:, 1]) + hm[8]
    assert zn.dtype == np.float32 and np.flatnonzero(zn == 0).tolist() == [16] and xi[16, 0] == 16.0
    with np.errstate(divide="ignore", invalid="ignore"):
        _, hd = S.heatmaps(p["pts"][16:17], 0, (ha, wa), p["inv_h"])
        _, hd_near = S.heatmaps(p["pts"][8:9], 0, (ha, wa), p["inv_h"])
    assert not hd.any() and hd_near.sum() == 1.0                      # x = 8: zn = 0.5, kept
    # the .5 landings: exact in float32, floors of both parities on both axes
    p = _pair(patch, "half")
    n = min(patch, 6) ** 2
    wp = S.warp_labels_f32(p["pts"][:n, :2].astype(np.int64), p["inv_h"])
    assert wp.dtype == np.float32 and np.array_equal(wp - np.floor(wp), np.full_like(wp, 0.5))
    for axis in (0, 1):
        assert set(np.floor(wp[:, axis]).astype(np.int64) % 2) == {0, 1}
    assert not np.array_equal(np.rint(wp), np.floor(wp + np.float32(0.5)))
    # landings exactly on x_max / y_max are kept, one past them dropped
    p = _pair(patch, "on_max")
    wp = S.warp_labels_f32(p["pts"][:6, :2].astype(np.int64), p["inv_h"])
    assert wp.tolist() == [[wa - 1, ha - 2], [wa - 2, ha - 1], [wa - 1, ha - 1], [wa, ha - 2], [wa - 2, ha], [wa - 3, ha - 3]]
    _, hd = S.heatmaps(p["pts"][:6], 0, (ha, wa), p["inv_h"])
    assert hd[ha - 2, wa - 1] == hd[ha - 1, wa - 2] == hd[ha - 1, wa - 1] == hd[ha - 3, wa - 3] == 1.0 and hd.sum() == 4.0
    assert p["win_dst"] == (ha - patch, wa - patch)
    # points inside the image and outside both windows
    p = _pair(patch, "far")
    xy = p["pts"][:5, :2].astype(np.int64)
    assert ((xy >= 0) & (xy < (wb, hb))).all()
    hs, hd = S.heatmaps(p["pts"][:5], 0, (hb, wb), p["inv_h"])
    assert hs.sum() == 5.0 and not S.crop(hs, p["win_src"], patch).any() and not S.crop(hd, p["win_dst"], patch).any()


@pytest.mark.parametrize("patch", (T.EDGE_PATCH, T.MANY_PATCH) + T.TINY_PATCHES)
def test_pole_window_holds_the_zero_of_w_and_both_clamps(patch):
    """The closed-form inverse is exact; W == 0 in the window of every pole pair (all of column 64 for the untilted one); the
    tilted pairs reach -2^31 and 2^31 - 1 wherever their window has a row below row 0."""
    for name, tilt in (("pole", 0.0), ("pole_neg", T.POLE_TILT), ("pole_pos", -T.POLE_TILT)):
        p = _pair(patch, name)
        assert np.array_equal(S.invert3(p["inv_h"]), np.array([1.0, 0, 0, 0, 1.0, 0, -1.0 / 64, -tilt, 1.0]))
        left = p["win_dst"][1]
        assert p["win_dst"][0] == 0 and left <= T.POLE_COLUMN < left + patch
        W, X, Y = T.pole_window_W(p, patch)
        col = T.POLE_COLUMN - left
        assert W[0, col] == 0.0 and X[0, col] == 0 and Y[0, col] == 0         # the W == 0 branch: the tap is (0, 0)
        if patch > 1:
            assert (W[:, :col] > 0).all() and (W[:, col + 1:] < 0).all()      # columns on both sides of the pole
        if tilt == 0.0:
            assert (W[:, col] == 0.0).all()
        elif patch > 1:
            sat = -2 ** 31 if tilt > 0 else 2 ** 31 - 1
            assert (X[1:, col] == sat).all() and (Y[1:, col] == sat).all()
    if patch > 1:                                                             # both saturations are inside the patches
        reached = np.concatenate([T.pole_window_W(_pair(patch, n), patch)[1].reshape(-1) for n in ("pole_neg", "pole_pos")])
        assert reached.min() == -2 ** 31 and reached.max() == 2 ** 31 - 1
    assert all(int(v) > 0 for v in T.edge_images()[0][0, 0])


def test_singular_matrices_have_a_determinant_of_exactly_zero():
    for name, m in T.SINGULAR.items():
        assert S.invert3(m) is None, name
        p = _pair(T.EDGE_PATCH, name)
        assert np.array_equal(p["inv_h"], m)
        assert not S.warp_perspective_u8(T.edge_images()[p["image"]], m).any()
    for patch in (T.EDGE_PATCH, T.MANY_PATCH):                                # y' = 0 / zn: the labels of zero_row land on row 0
        p = _pair(patch, "zero_row")
        _, hd = S.heatmaps(p["pts"], 0, T.EDGE_SHAPES[0], p["inv_h"])
        assert hd[0].any() and not hd[1:].any() and p["win_dst"][0] == 0
    assert S.crop(hd, _pair(T.EDGE_PATCH, "zero_row")["win_dst"], T.EDGE_PATCH).any()
    names = T.edge_names()
    for name in T.SINGULAR:                                                   # ordinary pairs on both sides
        i = names.index(name)
        for j in (i - 1, i + 1):
            assert S.invert3(T.edge_pairs(T.EDGE_PATCH)[j]["inv_h"]) is not None
    assert any(not r.any() for r in T.SINGULAR["zero_row"]) and all(r.any() for r in T.SINGULAR["rank_one"])


def test_many_pairs_cycle_every_edge():
    call = T.many_pairs_call()
    assert len(call["pairs"]) == T.MANY_PAIRS == 64 and call["patch"] == 8
    names = [p["name"] for p in call["pairs"]]
    assert set(names) == set(T.edge_names()) and names[:12] == T.edge_names()
    off = T.pack_call(call)["pts_offsets"]
    assert off[8] - off[7] == 1100 and off[41] - off[40] == 1100 and off[8] > T.LBL_THREADS and off[-1] == len(T.pack_call(call)["pts"])
    assert [names[i] for i in T.MANY_SPOT] == ["zero_row", "pole", "trunc", "rank_one"]
    assert all(len(p["pts"]) > T.MANY_TOP_K for p in call["pairs"])


# ---- B. balf_detector_loss -------------------------------------------------------------------------------------------------
def test_loss_planes_cross_one_wave_of_partials():
    for plane in T.LOSS_PLANES + T.LOSS_THIN + (T.LOSS_WORKLOAD,):
        assert T.loss_nblk(*plane) == T.LOSS_NBLK[plane]
    assert sorted(set(T.LOSS_NBLK.values())) == [63, 64, 65, 66, 128] and T.LOSS_WAVE == 64
    assert [h * w for h, w in T.LOSS_PLANES] == [16128, 16129, 16384, 16510]


def test_a_fully_masked_image_has_the_epsilon_denominator():
    hc, wc = T.LOSS_PLANES[3]
    c = T.loss_case(hc, wc, True)
    assert c["logits"].shape[0] == 3 and not c["valid_mask"][2].any() and c["valid_mask"][:2].any()
    vm = T.valid_cells(c["valid_mask"])
    den = (vm.astype(np.float32) + np.float32(1e-6)).astype(np.float64).sum(axis=1)
    assert den[2] == hc * wc * float(np.float32(1e-6))                        # exact: 16510 equal float32 terms in float64
    assert 0 < (~vm[0]).sum() < hc * wc // 4                                  # the drawn mask removes some cells, not most
    plain = T.loss_case(hc, wc, False)
    assert plain["valid_mask"] is None and plain["noise"] is None


def test_late_cells_lie_in_workgroups_past_the_first_wave_of_partials():
    c = T.late_cells_case()
    hc, wc = T.LATE_PLANE
    vm = T.valid_cells(c["valid_mask"])
    cells = np.flatnonzero(vm[0])
    assert T.LATE_FIRST_CELL == 64 * 256 and len(cells) == hc * wc - T.LATE_FIRST_CELL == 126
    assert cells.min() >= T.LATE_FIRST_CELL and (cells // T.LOSS_THREADS >= T.LOSS_WAVE).all()
    assert set(np.unique(c["valid_mask"][0].numpy())) == {0.0, 1.0}
    assert vm[1].sum() > hc * wc // 2 and vm[1][:T.LATE_FIRST_CELL].any()
    r = D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"])
    assert float(r["per_image"][0]) > 1.0 and np.isfinite(r["per_image"]).all()      # the late cells carry the whole loss
    assert not r["grad"][0].reshape(65, -1)[:, :T.LATE_FIRST_CELL].any() and r["grad"][0].reshape(65, -1)[:, cells].all()
    assert torch.equal(c["valid_mask"][0, 0, ::8, ::8].reshape(-1) != 0, torch.from_numpy(vm[0]))
