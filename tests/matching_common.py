"""The matching score of the HSequences evaluation restated with NumPy, written from the definitions alone;
shared by tests/test_matching_host.py and tests/test_matching_gpu.py.

For one pair after detection:
  1. kept lists: the common-region filter (both masks, ``mask[rint(y) - 1, rint(x) - 1]`` with NumPy's indexing, an index
     NumPy rejects drops the row, a singular homography keeps nothing), kept rows in order; the kept destination rows warped
     into the source image;
  2. each kept row takes the descriptor of the row it came from;
  3. ``match_smnn`` of the kept source descriptors against the kept destination descriptors -> M pairs (i, j);
  4. e = sqrt(dx*dx + dy*dy) in float64 between S[i] and D'[j];
  5. correct[k] = #(e <= t_k);
  6. the record fields.
"""
import numpy as np
import torch

from oracle import oracle as O


def kept_rows(pts, mask):
    """Indices of the rows (x, y, ...) inside ``mask``, in order."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    h, w = mask.shape
    keep = []
    for r, (x, y) in enumerate(pts[:, :2]):
        iy, ix = int(np.rint(y)) - 1, int(np.rint(x)) - 1
        if -h <= iy < h and -w <= ix < w and mask[iy, ix] != 0:
            keep.append(r)
    return np.asarray(keep, dtype=np.int64)


def kept_lists(src, dst, hm, shape_src, shape_dst):
    """-> (S [ks,4], D' [kd,4], index of each S row in src, index of each D' row in dst)."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 4), np.asarray(dst, dtype=np.float64).reshape(-1, 4)
    try:
        mask_src, mask_dst = O.create_common_region_masks(hm, shape_src, shape_dst, numpy_inverse=False)
    except np.linalg.LinAlgError:
        none = np.zeros(0, dtype=np.int64)
        return np.zeros((0, 4)), np.zeros((0, 4)), none, none
    i_s, i_d = kept_rows(src, mask_src), kept_rows(dst, mask_dst)
    return src[i_s], O.apply_homography_to_points(dst[i_d], hm), i_s, i_d


def reprojection_errors(s_rows, d_rows, matches):
    """e per match (i, j); NaN for a match with an index outside the lists."""
    s_rows, d_rows = np.asarray(s_rows, dtype=np.float64), np.asarray(d_rows, dtype=np.float64)
    e = np.full(len(matches), np.nan)
    for k, (i, j) in enumerate(np.asarray(matches, dtype=np.int64).reshape(-1, 2)):
        if 0 <= i < len(s_rows) and 0 <= j < len(d_rows):
            dx, dy = s_rows[i, 0] - d_rows[j, 0], s_rows[i, 1] - d_rows[j, 1]
            e[k] = np.sqrt(dx * dx + dy * dy)
    return e


def correct_counts(e, thresholds):
    e = np.asarray(e, dtype=np.float64)
    return np.asarray([int(np.count_nonzero(e <= float(t))) for t in thresholds], dtype=np.int64)


def ratio(num, den):
    return 0.0 if int(den) == 0 else float(np.float64(int(num)) / np.float64(int(den)))


def matching_record(s_rows, d_rows, desc_s, desc_d, th=0.99, thresholds=range(1, 11), pixel_threshold=5):
    """The record fields of one pair from its kept lists and the descriptors of the kept rows."""
    thresholds = [float(t) for t in thresholds]
    k_star = thresholds.index(float(pixel_threshold))
    ks, kd = len(s_rows), len(d_rows)
    if ks and kd:
        _, idx = O.match_smnn(torch.from_numpy(np.ascontiguousarray(desc_s, dtype=np.float32)),
                              torch.from_numpy(np.ascontiguousarray(desc_d, dtype=np.float32)), th)
        matches = idx.numpy().reshape(-1, 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            rep = O.compute_repeatability(s_rows, d_rows)
        possible = int(rep["possible_matches"])
    else:
        matches, rep, possible = np.zeros((0, 2), dtype=np.int64), None, 0
    e = reprojection_errors(s_rows, d_rows, matches)
    correct = correct_counts(e, thresholds)
    m = len(matches)
    avg = 0.0
    for c in correct:                                            # summed in ascending k, then divided by T
        avg = avg + ratio(c, m)
    return {"num_features": (ks, kd), "valid": int(ks > 0 and kd > 0), "num_mutual_corresp": m,
            "num_matches": int(correct[k_star]), "correct": correct, "mma": ratio(correct[k_star], m),
            "mma_corr": ratio(correct[k_star], possible), "avg_mma": avg / float(len(thresholds)),
            "match_idx": matches, "match_err": e, "possible_matches": possible, "repeatability": rep}


def pair_record(src, dst, desc_src, desc_dst, hm, shape_src, shape_dst, **kw):
    """Steps 1-6 from the detected rows and the per-image descriptors of one pair."""
    s_rows, d_rows, i_s, i_d = kept_lists(src, dst, hm, shape_src, shape_dst)
    return matching_record(s_rows, d_rows, np.asarray(desc_src)[i_s], np.asarray(desc_dst)[i_d], **kw)
