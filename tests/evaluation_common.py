"""Shared by tests/test_evaluation_edges_host.py and tests/test_evaluation_edges_gpu.py: float64 NumPy
references of the evaluation leg's operations -- the circle overlaps of compute_repeatability, the common-region point
filter, the match verification, the point selection of check_val_repeatability -- and the input generators that put a list
length, a pair count or a K just before, on and just past a chunk boundary of the kernels.  Nothing here needs a GPU; the
host test pins the references to the recorded goldens and the generators to the properties the GPU tests rely on."""
import functools

import numpy as np

from oracle import oracle as O
from tests import resize_repeat_common as RR
from tests import val_repeat_common as V

THR_MARGIN = 1e-9            # no generated overlap lies this close to 1 - overlap_err (a last-bit acos difference cannot matter)
FAR = 1.0e4                  # garbage rows / background coordinates stay below this


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- compute_repeatability: the overlaps ------------------------------------------------------------------------------------
def overlaps_np(src, dst, eps=1e-6, radious_size=30.0):
    """-> (single, multi) [ns, nd] float64: the two overlap matrices of oracle.compute_repeatability (the same expressions)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    dx = src[:, None, 0] - dst[None, :, 0]
    dy = src[:, None, 1] - dst[None, :, 1]
    dist = (dx ** 2 + dy ** 2) ** 0.5
    near = dist <= 4 * radious_size
    rr, rd = np.broadcast_arrays(src[:, None, 2], dst[None, :, 2])
    factor = radious_size / (np.maximum(rr, rd) + np.finfo(float).eps)
    inter = O._circle_intersection(factor * rr, factor * rd, dist)
    union = np.pi * (factor * rr) ** 2 + np.pi * (factor * rd) ** 2 - inter + eps
    multi = np.where(near, inter / union, 0.0)
    inter = O._circle_intersection(radious_size, radious_size, dist)
    union = np.pi * radious_size ** 2 + np.pi * radious_size ** 2 - inter + eps
    single = np.where(near, inter / union, 0.0)
    return single, multi


def candidate_counts(src, dst, overlap_err=0.4, **kw):
    """-> (per source row [ns, 2], totals [2]): the pairs whose (single, multi) overlap reaches 1 - overlap_err."""
    if len(src) == 0 or len(dst) == 0:
        return np.zeros((len(src), 2), np.int64), np.zeros(2, np.int64)
    s, m = overlaps_np(src, dst, **kw)
    rows = np.stack([(s >= 1 - overlap_err).sum(axis=1), (m >= 1 - overlap_err).sum(axis=1)], axis=1)
    return rows, rows.sum(axis=0)


def threshold_margin(src, dst, overlap_err=0.4, **kw):
    """The smallest |overlap - (1 - overlap_err)| over both matrices (inf for an empty side)."""
    if len(src) == 0 or len(dst) == 0:
        return np.inf
    s, m = overlaps_np(src, dst, **kw)
    return float(min(np.abs(s - (1 - overlap_err)).min(), np.abs(m - (1 - overlap_err)).min()))


def oracle_repeatability(src, dst, **kw):
    with np.errstate(invalid="ignore", divide="ignore"):
        return O.compute_repeatability(src, dst, **kw)


def pack(lists, n_max, rng, cols=4):
    """host row lists -> ([P, n_max, cols] float64 with garbage past each count, counts [P] int32)."""
    out = rng.uniform(-FAR, FAR, (len(lists), max(n_max, 1), cols))
    for k, a in enumerate(lists):
        if len(a):
            out[k, :len(a)] = np.asarray(a, dtype=np.float64)[:, :cols]
    return np.ascontiguousarray(out[:, :n_max]), np.asarray([len(a) for a in lists], np.int32)


def _background(rng, n, cell=400.0):
    """n rows (x, y, radius, score) on a jittered grid `cell` apart, far from the origin quadrant the plants use: more than
    4 * 30 from each other and from every planted row, so they carry no candidate."""
    side = int(np.ceil(np.sqrt(max(n, 1))))
    k = np.arange(n)
    xy = np.stack([(k % side) * cell, (k // side) * cell], axis=1) + 5000.0 + rng.uniform(-20, 20, (n, 2))
    return np.concatenate([xy, rng.choice([1.0, 1.5, 2.0], (n, 1)), rng.uniform(0, 1, (n, 1))], axis=1)


# ---- 1. the row scan across chunks ------------------------------------------------------------------------------------------
ROW_SCAN_NS = (1023, 1024, 1025, 2049, 3)
ROW_SCAN_ND = (5, 7, 3, 4, 2049)
BOUNDARY_ROWS = (1022, 1023, 1024, 1025, 2047, 2048)
SPOT_A, SPOT_B = np.array([300.0, 300.0]), np.array([900.0, 300.0])


@functools.lru_cache(maxsize=None)
def row_scan_pairs():
    """The five pairs of part 1.  Pairs 0..3 (long source list, tiny destination list): destination row 0 sits at spot A, the
    others at spot B, 600 apart; a source row near A has one candidate per scale it qualifies for, one near B has nd - 1.
    The boundary rows alternate A, B, A, B, A, B, so the counts differ across 1023|1024 and 2047|2048; every 37th row is
    planted too (alternating), so the running sums are not flat; radius 2 rows (every third plant) are single-scale
    candidates only (equal circles of radius 30 against circles of 30 and 15).  Everything else is background.  Pair 4 is the
    transpose: three source rows at A, B and far away, 2049 destination rows with plants at rows 0, 63, 64, 1023, 1024, 2048."""
    rng = np.random.default_rng(4101)
    pairs = []
    for ns, nd in zip(ROW_SCAN_NS[:4], ROW_SCAN_ND[:4]):
        src = _background(rng, ns)
        dst = np.zeros((nd, 4))
        dst[:, :2] = SPOT_B + rng.uniform(-1.0, 1.0, (nd, 2))
        dst[0, :2] = SPOT_A + rng.uniform(-1.0, 1.0, 2)
        dst[:, 2], dst[:, 3] = 1.0, rng.uniform(0, 1, nd)
        plants = sorted(set(range(11, ns, 37)) | {r for r in BOUNDARY_ROWS if r < ns})
        for k, r in enumerate(plants):
            spot = (SPOT_A, SPOT_B)[BOUNDARY_ROWS.index(r) % 2 if r in BOUNDARY_ROWS else k % 2]
            src[r, :2] = spot + rng.uniform(-4, 4, 2)
            src[r, 2] = 1.0 if r in BOUNDARY_ROWS or k % 3 else 2.0
        pairs.append(frozen(src, dst))
    ns, nd = ROW_SCAN_NS[4], ROW_SCAN_ND[4]
    src = np.array([[*SPOT_A, 1.0, 0.5], [*SPOT_B, 1.0, 0.25], [5000.0, 100.0, 1.0, 0.75]])
    dst = _background(rng, nd)
    for k, j in enumerate((0, 63, 64, 1023, 1024, 2048)):
        dst[j, :2] = (SPOT_A, SPOT_B)[k % 2] + rng.uniform(-4, 4, 2)
        dst[j, 2] = 1.0 if k % 3 else 1.25
    pairs.append(frozen(src, dst))
    return tuple(pairs)


# ---- 2. the pair scan across chunks -----------------------------------------------------------------------------------------
PAIR_SCAN_P, PAIR_SCAN_N = 2050, 6
PAIR_SCAN_NONEMPTY = (1023, 1024, 1025, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def pair_scan_pairs():
    """2050 pairs of 0..6 rows per side inside a 25 x 25 square (most rows overlap some row of the other side); a fifth of the
    pairs has an empty side; the pairs around 1024 and 2048 have rows on both sides and a planted coincident pair."""
    rng = np.random.default_rng(4102)
    pairs = []
    for p in range(PAIR_SCAN_P):
        ns, nd = (int(v) for v in rng.integers(0, PAIR_SCAN_N + 1, 2))
        if p in PAIR_SCAN_NONEMPTY:
            ns, nd = max(ns, 1 + p % 3), max(nd, 2)
        elif p % 5 == 0:
            ns, nd = (0, nd) if p % 10 else (ns, 0)
        src = np.concatenate([rng.uniform(0, 25, (ns, 2)), rng.choice([1.0, 1.5, 2.0], (ns, 1)), rng.uniform(0, 1, (ns, 1))], axis=1)
        dst = np.concatenate([rng.uniform(0, 25, (nd, 2)), rng.choice([1.0, 1.5, 2.0], (nd, 1)), rng.uniform(0, 1, (nd, 1))], axis=1)
        if p in PAIR_SCAN_NONEMPTY:
            dst[0, :2] = src[0, :2] + rng.uniform(0.5, 2.0, 2)
            dst[0, 2] = src[0, 2]
        pairs.append(frozen(src, dst))
    return tuple(pairs)


# ---- 3. the overflow boundary -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow_pairs():
    """Six small pairs, each with candidates in both scales and different counts in the two."""
    from tests.golden import cases
    return tuple(frozen(*cases.repeat_inputs(dict(ns=30 + 7 * k, nd=50 - 5 * k, seed=300 + k, planted=20 + k, spread=150.0)))
                 for k in range(6))


# ---- 4. the sort and the greedy walk ----------------------------------------------------------------------------------------
EQUAL_KEY_SHAPES = ((1, 1), (1, 63), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (33, 33), (45, 46))   # n = a * b


def equal_key_pair(a, b):
    """a coincident source rows, b coincident destination rows 5 pixels away (a 3-4-5 triangle), one radius: every overlap is
    the same number, in both scales."""
    src = np.tile([100.0, 200.0, 1.5, 0.5], (a, 1))
    dst = np.tile([103.0, 204.0, 1.5, 0.5], (b, 1))
    return src, dst


# (a, b, the (dx, dy) of the destination positions in turn, the destination radii in turn): all source rows coincide, radius 1
FEW_KEY_CASES = (
    (7, 9, ((3, 4), (6, 8)), (1.0,)),
    (40, 30, ((3, 4), (0, 7), (6, 8)), (1.0,)),
    (33, 64, ((0, 2), (0, 3)), (1.0,)),
    (12, 100, ((3, 4), (6, 8), (0, 6)), (1.0, 1.25)),
    (64, 17, ((1, 0), (0, 9)), (1.0,)),
    (5, 70, ((8, 6), (0, 1), (0, 4)), (1.0, 1.1, 1.0)),
)


def few_key_pair(case):
    a, b, offsets, radii = case
    src = np.tile([500.0, 400.0, 1.0, 0.5], (a, 1))
    dst = np.zeros((b, 4))
    for j in range(b):
        dx, dy = offsets[j % len(offsets)]
        dst[j] = (500.0 + dx, 400.0 + dy, radii[j % len(radii)], 0.5)
    return src, dst


def differing_nibbles(keys):
    """How many of the 16 four-bit digits of the 64-bit `keys` are NOT the same in every key: the passes rep_sort_pairs runs."""
    k = np.asarray(keys, np.float64).view(np.uint64)
    return sum(int(len(np.unique((k >> np.uint64(s)) & np.uint64(15))) > 1) for s in range(0, 64, 4))


def candidate_keys(src, dst, overlap_err=0.4):
    """-> (single keys, multi keys): the overlaps that reach the threshold, in flat order."""
    s, m = overlaps_np(src, dst)
    return s[s >= 1 - overlap_err], m[m >= 1 - overlap_err]


WORD_EDGES = (31, 32, 33, 64, 65)


def word_edge_pair(ns, nd):
    """Spots 300 apart, one to two rows of each side at a spot (assigned through random permutations), every row at its own
    offset from the spot: small clusters whose overlaps are all distinct, so rows compete for a partner and the walk has to
    consult the visited bit of every index, 31, 32, 63 and 64 included."""
    rng = np.random.default_rng([4104, ns, nd])
    spots = min(ns, nd) // 2 + 1
    grid = np.stack([(np.arange(spots) % 8) * 300.0, (np.arange(spots) // 8) * 300.0], axis=1) + 100.0
    src = np.zeros((ns, 4))
    dst = np.zeros((nd, 4))
    src[:, :2] = grid[rng.permutation(ns) % spots] + np.stack([rng.permutation(ns) * (9.0 / ns) + 0.5, np.zeros(ns)], axis=1)
    dst[:, :2] = grid[rng.permutation(nd) % spots] + np.stack([np.zeros(nd), rng.permutation(nd) * (9.0 / nd) + 0.25], axis=1)
    src[:, 2], dst[:, 2] = rng.choice([1.0, 1.25], ns), rng.choice([1.0, 1.25], nd)
    src[:, 3], dst[:, 3] = rng.uniform(0, 1, ns), rng.uniform(0, 1, nd)
    # the last two rows of both sides share a spot of their own: (ns - 1, nd - 1) is taken first, (ns - 2, nd - 1) and
    # (ns - 1, nd - 2) are then refused on the visited bit of the LAST index of a side, (ns - 2, nd - 2) is taken
    src[-2:] = [[5003.0, 5000.0, 1.0, 0.5], [5001.0, 5000.0, 1.0, 0.5]]
    dst[-2:] = [[5000.0, 5004.0, 1.0, 0.5], [5000.0, 5000.0, 1.0, 0.5]]
    return src, dst


MAX_ROWS = 65536


@functools.lru_cache(maxsize=None)
def limit_pair(long_side):
    """(65536, 2) for long_side 0, (2, 65536) for 1: background rows with plants at the first rows, around every 1024-row
    chunk edge that a bitmap word or a scan chunk ends on, and at the last two rows."""
    rng = np.random.default_rng(4105 + long_side)
    long = _background(rng, MAX_ROWS, cell=130.0)
    short = np.array([[*SPOT_A, 1.0, 0.5], [*SPOT_B, 1.0, 0.25]])
    for k, r in enumerate((0, 1, 1023, 1024, 32767, 32768, 65503, 65504, 65534, 65535)):
        long[r, :2] = (SPOT_A, SPOT_B)[k % 2] + rng.uniform(-4, 4, 2)
        long[r, 2] = 1.0 if k % 3 else 1.25
    return frozen(short, long) if long_side else frozen(long, short)


# ---- 5. the common-region filter --------------------------------------------------------------------------------------------
def check_common_points_np(pts_xy, mask):
    """check_common_points (repeatability_tools.py:8-13) on (x, y) rows: the rows with mask[round(y) - 1, round(x) - 1] != 0,
    round half to even, a negative index wrapping like NumPy's; a row whose index NumPy would reject (NaN, inf, outside
    [-n, n)) is dropped, which is the batched filter's documented rule (the reference raises there)."""
    h, w = mask.shape
    with np.errstate(invalid="ignore"):
        ry, rx = np.rint(pts_xy[:, 1]) - 1.0, np.rint(pts_xy[:, 0]) - 1.0
        ok = (ry >= -h) & (ry < h) & (rx >= -w) & (rx < w)
    keep = np.zeros(len(pts_xy), bool)
    iy, ix = ry[ok].astype(np.int64), rx[ok].astype(np.int64)
    keep[ok] = mask[iy, ix] != 0
    return np.flatnonzero(keep)


def common_points_ref(src, dst, h, shapes):
    """One pair of balf_common_points_index_batch -> (kept source rows, warped kept destination rows, source index,
    destination index).  A singular h and a shape with a non-positive entry keep nothing (include/balf_hip.h)."""
    empty = (np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int64))
    if min(shapes) <= 0:
        return empty
    try:
        ms, md = O.create_common_region_masks(h, shapes[:2], shapes[2:], numpy_inverse=False)
    except np.linalg.LinAlgError:
        return empty
    i_s = check_common_points_np(src[:, :2], ms) if len(src) else np.zeros(0, np.int64)
    i_d = check_common_points_np(dst[:, :2], md) if len(dst) else np.zeros(0, np.int64)
    return src[i_s], O.apply_homography_to_points(dst[i_d], h), i_s, i_d


SINGULAR_H = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])      # det = 1 * 4 - 2 * 2 + 3 * 0 = 0 exactly
COMMON_N_MAX = 513


def _inside(rng, n, h, w):
    """n rows whose rounded (x, y) lies in [16, w - 15] x [16, h - 15]: mask index in [15, n - 16], inside the frame."""
    return np.stack([rng.uniform(15.6, w - 14.6, n), rng.uniform(15.6, h - 14.6, n), rng.choice([1.0, 1.5, 2.0], n),
                     rng.uniform(0, 1, n)], axis=1)


@functools.lru_cache(maxsize=None)
def common_cases():
    """-> list of dict(name, src, dst, ns, nd, h, shapes): the pairs of part 5.  ns / nd are the counts handed to the device
    (the lists hold the rows the clamped counts reach)."""
    rng = np.random.default_rng(4106)
    eye = np.eye(3)
    out = []

    def add(name, src, dst, h, shapes, ns=None, nd=None):
        out.append(dict(name=name, src=src, dst=dst, h=np.asarray(h, np.float64), shapes=tuple(shapes),
                        ns=len(src) if ns is None else ns, nd=len(dst) if nd is None else nd))

    for n_s, n_d in ((255, 513), (256, 257), (257, 256), (513, 255)):
        add(f"inside_{n_s}_{n_d}", _inside(rng, n_s, 100, 140), _inside(rng, n_d, 100, 140), eye, (100, 140, 100, 140))
    small = np.stack([rng.uniform(0, 29, 40), rng.uniform(0, 29, 40), np.ones(40), rng.uniform(0, 1, 40)], axis=1)
    add("30x30", small, small[::-1].copy(), eye, (30, 30, 30, 30))
    one = np.array([[16.0, 16.0, 1.0, 0.5], [15.0, 15.0, 1.0, 0.25], [16.4, 15.6, 2.0, 0.75], [17.0, 16.0, 1.0, 0.1],
                    [16.0, 17.0, 1.0, 0.2], [16.5, 16.5, 1.0, 0.3]])         # 16.5 rounds to 16 (half to even)
    add("31x31", one, one[::-1].copy(), eye, (31, 31, 31, 31))
    good = _inside(rng, 24, 100, 140)
    bad = good.copy()
    bad[1::3, 0] = [np.nan, np.inf, -np.inf, 1e300, -1e300, -0.4, 20.0, 20.0]
    bad[2::3, 1] = [20.0, 20.0, np.nan, -np.inf, np.inf, -1e300, 1e300, -0.4]
    add("bad_coordinates", bad, bad[::-1].copy(), eye, (100, 140, 100, 140))
    add("counts_clamped", _inside(rng, COMMON_N_MAX, 100, 140), _inside(rng, COMMON_N_MAX, 100, 140), eye, (100, 140, 100, 140),
        ns=-5, nd=COMMON_N_MAX + 7)
    add("singular", _inside(rng, 50, 100, 140), _inside(rng, 60, 100, 140), SINGULAR_H, (100, 140, 100, 140))
    add("zero_shape", _inside(rng, 50, 100, 140), _inside(rng, 60, 100, 140), eye, (100, 0, 100, 140))
    add("negative_shape", _inside(rng, 50, 100, 140), _inside(rng, 60, 100, 140), eye, (100, 140, -100, 140))
    frame = _inside(rng, 70, 100, 140)
    frame[:, 0] = rng.uniform(0.0, 14.4, 70)                                 # every source row in the zeroed frame
    add("one_side_empty", frame, _inside(rng, 80, 100, 140), eye, (100, 140, 100, 140))
    from tests.golden import cases
    wide = np.stack([rng.uniform(0, 319, 400), rng.uniform(0, 239, 400), rng.choice([1.0, 2.0], 400), rng.uniform(0, 1, 400)], axis=1)
    add("perspective", wide, wide[rng.permutation(400)][:300], cases.HOMOGRAPHY, (240, 320, 240, 320))
    for c in out:
        frozen(c["src"], c["dst"], c["h"])
    return tuple(out)


def effective_rows(case):
    """The rows a case's clamped counts reach."""
    ns, nd = (int(np.clip(case[k], 0, COMMON_N_MAX)) for k in ("ns", "nd"))
    return case["src"][:ns], case["dst"][:nd]


# ---- 6. the match verification ----------------------------------------------------------------------------------------------
TRIANGLES = ((3, 4, 5.0), (6, 8, 10.0), (5, 12, 13.0))
BAD_INDEX = 2 ** 31 - 1


def below(v):
    return float(np.nextafter(v, -np.inf))


THRESHOLDS_16 = (0.0, 1.0, 4.0, below(5.0), 5.0, 7.0, below(10.0), 10.0, 11.0, below(13.0), 13.0, 20.0, 50.0, 100.0, 1e3, 1e6)
THRESHOLDS_1 = ((5.0,), (below(5.0),))
MATCH_CAPS = (1, 255, 256, 257, 1000)
MATCH_N_MAX = 1000


def match_accuracy_np(src, dst, kept, match_idx, match_count, thresholds):
    """balf_match_accuracy_batch restated -> (err [P, cap] float64, correct [P, T] int64)."""
    p, cap = match_idx.shape[:2]
    err = np.full((p, cap), np.nan)
    correct = np.zeros((p, len(thresholds)), np.int64)
    for q in range(p):
        ks, kd = (int(np.clip(kept[q, s], 0, n)) for s, n in ((0, src.shape[1]), (1, dst.shape[1])))
        m = int(np.clip(match_count[q], 0, cap))
        i, j = match_idx[q, :m, 0].astype(np.int64), match_idx[q, :m, 1].astype(np.int64)
        ok = (i >= 0) & (i < ks) & (j >= 0) & (j < kd)
        dx = src[q, i[ok], 0] - dst[q, j[ok], 0]
        dy = src[q, i[ok], 1] - dst[q, j[ok], 1]
        e = np.full(m, np.nan)
        e[ok] = np.sqrt(dx * dx + dy * dy)
        err[q, :m] = e
        with np.errstate(invalid="ignore"):
            correct[q] = [(e <= t).sum() for t in thresholds]
    return err, correct


@functools.lru_cache(maxsize=None)
def match_case(cap):
    """Six pairs for one cap -> dict(src, dst [6, 1000, 4], kept [6, 2], match_idx [6, cap, 2], match_count [6]).  Integer
    coordinates; match k of a pair joins source row i_k and destination row j_k (both drawn without replacement) that lie a
    Pythagorean triple apart (errors exactly 5, 10, 13), coincide (0) or sit a unit diagonal apart (sqrt 2).  Pair 0: a count
    below cap; 1: above cap (clamped); 2: negative (clamped to 0); 3: kept counts above n_max; 4: count == cap with the four
    bad indices (-1, ks, kd, 2^31 - 1) in turn at every seventh slot; 5: kept counts that cut the lists short, so that some
    matches point past them."""
    rng = np.random.default_rng([4107, cap])
    p, n = 6, MATCH_N_MAX
    src = np.concatenate([rng.integers(0, 2000, (p, n, 2)).astype(np.float64), np.ones((p, n, 1)), rng.uniform(0, 1, (p, n, 1))], axis=2)
    dst = np.concatenate([rng.integers(5000, 7000, (p, n, 2)).astype(np.float64), np.ones((p, n, 1)), rng.uniform(0, 1, (p, n, 1))], axis=2)
    idx = np.zeros((p, cap, 2), np.int32)
    offsets = [(sx * a, sy * b) for a, b, _ in TRIANGLES for sx in (1, -1) for sy in (1, -1)] + \
              [(sx * b, sy * a) for a, b, _ in TRIANGLES for sx in (1, -1) for sy in (1, -1)] + [(0, 0), (1, 1), (-1, 1)]
    for q in range(p):
        i, j = rng.permutation(n)[:cap], rng.permutation(n)[:cap]
        idx[q, :, 0], idx[q, :, 1] = i, j
        off = np.asarray(offsets, np.float64)[rng.integers(0, len(offsets), cap)]
        dst[q, j, :2] = src[q, i, :2] + off
    kept = np.full((p, 2), n, np.int32)
    kept[3] = (n + 5, n + 900)
    kept[5] = (n // 2, n // 3)
    count = np.asarray([max(cap - 3, 0) if cap > 1 else 1, cap + 9, -3, cap, cap, cap], np.int32)
    bad = (-1, kept[4, 0], kept[4, 1], BAD_INDEX)
    for k in range(0, cap, 7):
        idx[4, k, (k // 7) % 2] = bad[(k // 7) % 4]
    return dict(zip(("src", "dst", "kept", "match_idx", "match_count"), frozen(src, dst, kept, idx, count)))


# ---- 7. the resize protocol beyond one LDS tile -----------------------------------------------------------------------------
MIN_TILE = 1024
RESIZE_H = np.array([[1.01, 0.02, -3.0], [-0.015, 0.99, 2.0], [2e-5, -1e-5, 1.0]])
RESIZE_SHAPE = (3600, 3600)
RESIZE_THRESH = 3.0
# (K, rows on the side above K, rows on the side below K), each run with the long side as source and as destination
RESIZE_CASES = ((1024, 1300, 1000), (1025, 1241, 1011), (2049, 2300, 1500), (3000, 3217, 2500))


@functools.lru_cache(maxsize=None)
def resize_case(k, n_above, n_below, long_is_src):
    """-> (src rows, dst rows) (row, col, prob): points spread over 3400 x 3400 (an unplanted nearest neighbour is ~30 pixels
    away), a third of the short side's rows planted at most 1.7 pixels from a row of the long side under RESIZE_H, probs distinct.
    The LAST row of the long side has the highest prob (it is kept, as the last kept row) and is the partner of the LAST row
    of the short side: each is the other's nearest neighbour, at column n_col - 1 in both directions."""
    rng = np.random.default_rng([4108, k, int(long_is_src)])
    ns, nd = (n_above, n_below) if long_is_src else (n_below, n_above)
    src = np.stack([rng.uniform(100, 3400, ns), rng.uniform(100, 3400, ns), rng.permutation(ns) / ns + 0.001], axis=1)
    dst = np.stack([rng.uniform(100, 3400, nd), rng.uniform(100, 3400, nd), rng.permutation(nd) / nd + 0.001], axis=1)
    m = n_below // 3
    a, b = rng.permutation(ns - 1)[:m], rng.permutation(nd - 1)[:m]
    a, b = np.append(a, ns - 1), np.append(b, nd - 1)
    wc, wr = RR.warp_cols_rows(src[a, 1], src[a, 0], RESIZE_H)
    dst[b, 0], dst[b, 1] = wr + rng.uniform(-1.2, 1.2, m + 1), wc + rng.uniform(-1.2, 1.2, m + 1)
    (src if long_is_src else dst)[-1, 2] = 2.0
    return frozen(src, dst)


def resize_reference(src, dst, k, thresh=RESIZE_THRESH, h=RESIZE_H, shape=RESIZE_SHAPE):
    """-> (result dict, argmin column of every row minimum, of every column minimum, kept counts)."""
    res, min1, min2 = RR.resize_repeatability_np(src, dst, h, shape, shape, k, thresh)
    a, b = RR.kept_rows(src, dst, h, shape, shape, k)
    dy, dx = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    d2 = dy * dy + dx * dx
    none = np.zeros(0, np.int64)
    return res, (d2.argmin(axis=1) if len(b) else none, min1), (d2.argmin(axis=0) if len(a) else none, min2), (len(a), len(b))


@functools.lru_cache(maxsize=None)
def resize_case_reference(k, n_above, n_below, long_is_src):
    """resize_reference of a case of RESIZE_CASES, computed once."""
    return resize_reference(*resize_case(k, n_above, n_below, long_is_src), k)


def signed_zero_case():
    """40 rows a side, K = 20: ten rows of positive prob, then fifteen of prob -0.0, then fifteen of +0.0.  Equal probs keep
    the lower index, so rows 10..19 complete the cut -- exactly the rows whose partner lies 1 pixel away; the +0.0 rows have
    no partner within reach.  An order that puts -0.0 below +0.0 keeps rows 25..34 instead and counts ten matches fewer."""
    rng = np.random.default_rng(4109)
    n = 40
    prob = np.concatenate([rng.uniform(0.5, 1.0, 10), np.full(15, -0.0), np.full(15, 0.0)])
    src = np.stack([100.0 + 40.0 * np.arange(n), 200.0 + 7.0 * np.arange(n), prob], axis=1)
    dst = src.copy()
    dst[:25, 0] += 1.0
    dst[25:, 1] += 300.0
    return src, dst, np.eye(3), (2000, 2000), (2000, 2000), 20, 3.0


# ---- 8. the validation selection at large K ---------------------------------------------------------------------------------
VAL_KS = (1, 1023, 1024, 1025, 2048, 6000, 16384)
VAL_LEGS = (("window", 1), ("window", 3), ("window", 15), ("greedy", 0), ("greedy", 1))
VAL_SHAPES = (((128, 128), (128, 128)), ((96, 160), (128, 128)))
VAL_HS = (np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [0.0, 0.0, 1.0]]),
          np.array([[0.98, 0.03, 1.5], [-0.02, 1.01, 2.0], [2.0e-5, -1.0e-5, 1.0]]),
          np.array([[1.02, -0.01, -2.0], [0.015, 0.97, 3.0], [-1.0e-5, 3.0e-5, 1.0]]))
VAL_GONE = np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])       # no common region: both fallbacks
# two batches of P = 3: (map kind, homography)
VAL_BATCHES = ((("dense", VAL_HS[0]), ("levels", VAL_HS[1]), ("sparse", VAL_HS[2])),
               (("zero", VAL_HS[1]), ("dense", VAL_GONE), ("levels", VAL_HS[2])))


def val_map(kind, shape, rng):
    h, w = shape
    if kind == "zero":
        return np.zeros((h, w), np.float32)
    if kind == "levels":                                             # 8 levels: ties at every cut
        return (rng.integers(0, 8, (h, w)) / 8.0).astype(np.float32)
    if kind == "sparse":
        m = np.zeros((h, w), np.float32)
        at = rng.choice(h * w, 700, replace=False)
        m.ravel()[at] = rng.uniform(0.02, 1.0, 700).astype(np.float32)
        return m
    return (rng.random((h, w), dtype=np.float32) * np.float32(0.98) + np.float32(0.02))      # dense: every pixel a candidate


@functools.lru_cache(maxsize=None)
def val_batch(batch, shapes):
    """-> (prob_src [3, Hs, Ws], prob_dst [3, Hd, Wd] float32, h [3, 3, 3])."""
    rng = np.random.default_rng([4110, batch, shapes[0][0]])
    cfg = VAL_BATCHES[batch]
    return frozen(np.stack([val_map(kind, shapes[0], rng) for kind, _ in cfg]),
                  np.stack([val_map(kind, shapes[1], rng) for kind, _ in cfg]), np.stack([h for _, h in cfg]))


@functools.lru_cache(maxsize=None)
def val_masked_maps(batch, shapes, leg, nms_size):
    """Per pair of a batch: (masked NMS map of the source, of the destination) -- oracle_pair's pieces before the selection,
    computed once for every K."""
    ps, pd, hs = val_batch(batch, shapes)
    out = []
    for p in range(len(hs)):
        ms, md = O.create_common_region_masks(hs[p], ps[p].shape, pd[p].shape, numpy_inverse=False)
        out.append(frozen(np.multiply(V.oracle_nms_map(ps[p], nms_size, leg), ms),
                          np.multiply(V.oracle_nms_map(pd[p], nms_size, leg), md)))
    return tuple(out)


def val_select(masked, k):
    """get_point_coordinates(masked, num_points=k, 'xysr') from the oracle's pieces -> rows (x, y, 1, score)."""
    idx, sc = O.select_topk(masked, k)
    return O.points_xysr(idx, sc, masked.shape[1])
