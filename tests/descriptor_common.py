"""Plain float64 NumPy references of the descriptor leg (patch extraction and mutual ratio-test matching), the accuracy
contract of the fp32 matcher, and the inputs the edge tests share.  Nothing here touches the GPU or the library's kernels:
tests/test_descriptor_edges_host.py checks these references against oracle.match_smnn / oracle.extract_patches on easy
inputs, tests/test_descriptor_edges_gpu.py checks the HIP kernels against them at the hard ones.

Matcher contract: a computed squared distance is within

    delta(i, j) = 16 * 2^-24 * (|a_i| + |b_j|)^2

of the exact one.  The constant is not read off the kernel: a NumPy fp32 emulation of d^2 = |a|^2 + |b|^2 - 2 a.b stays below
4.6 * 2^-24 * (|a| + |b|)^2 for per-component noise 3e-5 .. 1e-2 and descriptor scales 1/64, 1 and 37; 16 leaves ~3.5x for
the different summation order of the MFMA.  A row is DECIDED when the fp64 gap between its best and second-best d^2 exceeds
2 delta: no computation inside the contract can pick another neighbour.  A ratio r = d1 / d2 carries the error
r * (delta / (2 d1^2) + delta / (2 d2^2))."""
import numpy as np

DELTA_C = 16.0 * 2.0 ** -24
PS = 32


# ---------------------------------------------------------------------------------------------------------------------
# matcher
# ---------------------------------------------------------------------------------------------------------------------
def dist2_f64(a, b, rows=64):
    """D2[i, j] = sum_k (a_ik - b_jk)^2 in float64 from the fp32 inputs (differences, not the expansion)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, a.shape[0], rows):
            d = a[i0:i0 + rows, None, :] - b[None, :, :]
            out[i0:i0 + rows] = np.einsum("ijk,ijk->ij", d, d)
    return out


class Side:
    """Nearest / second-nearest neighbour of every row of `d2m` (rows = queries), the oracle's way: a NaN distance sorts
    last (it is never a nearest nor a second-nearest neighbour while two comparable ones exist), ties go to the lowest
    index."""

    def __init__(self, d2m, qnorm, cnorm):
        n, m = d2m.shape
        self.n = n
        key = np.where(np.isnan(d2m), np.inf, d2m)
        order = np.argsort(key, axis=1, kind="stable")[:, :2] if m else np.zeros((n, 0), np.int64)
        rows = np.arange(n)
        self.nn = order[:, 0] if m else np.full(n, -1)
        self.d1 = d2m[rows, order[:, 0]] if m else np.full(n, np.nan)
        self.d2 = d2m[rows, order[:, 1]] if m > 1 else np.full(n, np.nan)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            self.ratio = np.sqrt(self.d1) / np.sqrt(self.d2)
            finite_c = cnorm[np.isfinite(cnorm)]
            cmax = finite_c.max() if finite_c.size else 0.0
            self.delta = DELTA_C * (qnorm + cmax) ** 2
            self.decided = np.isfinite(self.delta) & (self.d2 - self.d1 > 2.0 * self.delta)        # NaN compares false
            self.ratio_err = self.ratio * (self.delta / (2.0 * self.d1) + self.delta / (2.0 * self.d2))
        self.ratio_err = np.where(np.isfinite(self.ratio_err), self.ratio_err, np.inf)

    def passes(self, th):
        with np.errstate(invalid="ignore"):
            return self.ratio <= th

    def ratio_decided(self, th):
        with np.errstate(invalid="ignore"):
            return self.decided & (np.abs(self.ratio - th) > self.ratio_err)


class MatchRef:
    """The exhaustive fp64 reference of match_smnn(d1, d2, th): ratio test with <= in both directions, mutual check,
    dist = max of the two ratios, sorted by the index in d1; no matches when either side has fewer than two rows."""

    def __init__(self, d1, d2, th):
        d1, d2 = np.asarray(d1, np.float32), np.asarray(d2, np.float32)
        self.th = float(th)
        self.n1, self.n2 = d1.shape[0], d2.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            na = np.sqrt((d1.astype(np.float64) ** 2).sum(1))
            nb = np.sqrt((d2.astype(np.float64) ** 2).sum(1))
        dm = dist2_f64(d1, d2)
        self.rows, self.cols = Side(dm, na, nb), Side(dm.T.copy(), nb, na)
        idx, dist = [], []
        if self.n1 >= 2 and self.n2 >= 2:
            p1, p2 = self.rows.passes(th), self.cols.passes(th)
            for i in range(self.n1):
                j = int(self.rows.nn[i])
                if p1[i] and p2[j] and self.cols.nn[j] == i:
                    idx.append((i, j))
                    dist.append(max(self.rows.ratio[i], self.cols.ratio[j]))
        self.idx = np.asarray(idx, np.int64).reshape(-1, 2)
        self.dist = np.asarray(dist, np.float64)
        self._pass = self.rows.passes(th), self.cols.passes(th)
        self._rdec = self.rows.ratio_decided(th), self.cols.ratio_decided(th)

    def decided_share(self):
        """share of desc1 rows and of desc2 rows whose nearest neighbour no computation inside the contract can change"""
        return float(self.rows.decided.mean()), float(self.cols.decided.mean())

    def pair_state(self, i, j):
        """'match' / 'no' when every computation inside the contract agrees, else 'open'"""
        if self.n1 < 2 or self.n2 < 2:
            return "no"
        r, c = self.rows, self.cols
        if (r.decided[i] and r.nn[i] != j) or (c.decided[j] and c.nn[j] != i):
            return "no"
        (p1, p2), (rd, cd) = self._pass, self._rdec
        if r.decided[i] and rd[i] and not p1[i]:
            return "no"
        if c.decided[j] and cd[j] and not p2[j]:
            return "no"
        if r.decided[i] and c.decided[j] and rd[i] and cd[j] and r.nn[i] == j and c.nn[j] == i:
            return "match"
        return "open"

    def check(self, got_idx, got_dist, note=print):
        """got_idx [M,2], got_dist [M] from the code under test.  Decided matches must all be there, nothing may be there
        that is decidedly no match, the order is by i, and every dist of a pair with decided neighbours is within the ratio
        error of the reference's.  Returns (decided matches, open pairs reported)."""
        got_idx = np.asarray(got_idx, np.int64).reshape(-1, 2)
        got_dist = np.asarray(got_dist, np.float64).reshape(-1)
        assert got_idx.shape[0] == got_dist.shape[0]
        assert np.all(np.diff(got_idx[:, 0]) > 0), "matches are not sorted by the index in desc1 (or an index repeats)"
        assert len(set(got_idx[:, 1].tolist())) == got_idx.shape[0], "a desc2 index is matched twice"
        got = {(int(i), int(j)): float(d) for (i, j), d in zip(got_idx, got_dist)}
        for (i, j) in got:
            assert 0 <= i < self.n1 and 0 <= j < self.n2, f"match ({i}, {j}) outside {self.n1} x {self.n2}"
        ref = {(int(i), int(j)): float(d) for (i, j), d in zip(self.idx, self.dist)}
        n_decided = n_open = 0
        worst = 0.0
        for (i, j), d in ref.items():
            if self.pair_state(i, j) == "match":
                n_decided += 1
                assert (i, j) in got, f"decided match ({i}, {j}) of the fp64 reference is missing"
        for (i, j), d in got.items():
            state = self.pair_state(i, j)
            assert state != "no", f"({i}, {j}) is reported but is decidedly no match in the fp64 reference"
            n_open += state == "open"
            if self.rows.decided[i] and self.cols.decided[j] and self.rows.nn[i] == j and self.cols.nn[j] == i:
                want = max(self.rows.ratio[i], self.cols.ratio[j])
                tol = max(self.rows.ratio_err[i], self.cols.ratio_err[j])
                if np.isfinite(tol):
                    worst = max(worst, abs(d - want) / tol)
                    assert abs(d - want) <= tol, f"dist of ({i}, {j}): {d} vs {want}, allowed {tol}"
        note(f"  matches: reference {len(ref)} ({n_decided} decided), reported {len(got)} ({n_open} open); "
             f"worst dist error / allowed = {worst:.3f}")
        return n_decided, n_open


def unit_rows(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 128)).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _renorm(x):
    return (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


NEAR_N1, NEAR_N2, NEAR_SOURCES, NEAR_TH = 203, 331, 100, 0.8
NEAR_CASES = [(sigma, scale) for sigma in (1e-3, 1e-2) for scale in (1.0, 37.0, 1.0 / 64.0)]


def near_duplicate_case(sigma, scale, seed=11):
    """203 x 331 unit descriptors; 100 rows of desc1 have two near-duplicates each in desc2, at per-component noise sigma
    and 1.5 sigma (re-normalised after planting), at shuffled positions; the whole set times `scale`.  What an HSequences
    pair looks like to the matcher: d^2 = |a|^2 + |b|^2 - 2 a.b cancels to ~128 sigma^2."""
    rng = np.random.default_rng(seed)
    d1, d2 = unit_rows(NEAR_N1, seed + 1), unit_rows(NEAR_N2, seed + 2)
    src = rng.permutation(NEAR_N1)[:NEAR_SOURCES]
    dst = rng.permutation(NEAR_N2)[:2 * NEAR_SOURCES]
    for k, s in enumerate((sigma, 1.5 * sigma)):
        noise = rng.standard_normal((NEAR_SOURCES, 128))
        d2[dst[k::2]] = _renorm(d1[src].astype(np.float64) + s * noise)
    return (d1 * np.float32(scale)).astype(np.float32), (d2 * np.float32(scale)).astype(np.float32), src, dst


SWEEP_SHAPES = [(15, 17), (16, 16), (17, 33), (1, 2), (2, 1), (1025, 1040), (1100, 1100)]
SWEEP_TH = 0.95


def sweep_case(n1, n2):
    """Shapes around the 16-row / 16-column tiles and the 1024-row step of the mutual kernel.  min(n1, n2) // 2 noisy
    correspondences at shuffled positions; (1100, 1100): desc2 is a shuffled, lightly noised copy of desc1, so every row
    matches (count == cap)."""
    rng = np.random.default_rng(1000 * n1 + n2)
    d1 = unit_rows(n1, 3 * n1 + n2)
    if (n1, n2) == (1100, 1100):
        perm = rng.permutation(n1)
        d2 = _renorm(d1[perm].astype(np.float64) + 1e-2 * rng.standard_normal((n1, 128)))
        return d1, d2, perm
    d2 = unit_rows(n2, 5 * n1 + n2 + 1)
    m = min(n1, n2) // 2
    if m:
        src, dst = rng.permutation(n1)[:m], rng.permutation(n2)[:m]
        d2[dst] = _renorm(d1[src].astype(np.float64) + 0.05 * rng.standard_normal((m, 128)))
    return d1, d2, None


TIE_N1, TIE_N2 = 20, 37
TIE_PAIRS = [(3, 4), (5, 21), (8, 29), (10, 36)]      # (j, j+1), (j, j+16), (j, j+21), (an earlier column, n2-1)


def tie_case(seed=41):
    """Query i (i = 0..3) has two EXACT duplicates in desc2, at the column pairs above, at a non-zero distance (|noise| ~
    0.55): with th = 1.0 the ratio of the tied row is exactly 1 and passes, so the chosen column reaches the output.
    (j, j+16) is the same lane in two column tiles (best_insert), the others are two lanes (best_merge)."""
    rng = np.random.default_rng(seed)
    d1, d2 = unit_rows(TIE_N1, seed + 1), unit_rows(TIE_N2, seed + 2)
    for i, (ja, jb) in enumerate(TIE_PAIRS):
        row = _renorm(d1[i:i + 1].astype(np.float64) + 0.05 * rng.standard_normal((1, 128)))[0]
        d2[ja] = row
        d2[jb] = row
    return d1, d2


# ---------------------------------------------------------------------------------------------------------------------
# patches
# ---------------------------------------------------------------------------------------------------------------------
def level_f64(h, w, scale):
    """level = clamp(floor(log2(2 s / PS)), 0, max(0, min(H, W) // PS - 1)), s = sqrt(scale^2 + 1e-10), in float64"""
    s = np.sqrt(np.float64(scale) ** 2 + 1e-10)
    return int(np.clip(np.floor(np.log2(2.0 * s / PS)), 0.0, max(0, min(h, w) // PS - 1)))


def level_f32(h, w, scale):
    """the same formula with every operation in fp32, as the library's host code states it"""
    f = np.float32
    sc = f(scale)
    s = np.sqrt(f(sc * sc + f(1e-10)))
    lv = np.floor(np.log2(f(f(2.0) * s) / f(PS)))
    hi = f(max(0, min(h, w) // PS - 1))
    return int(min(max(lv, f(0.0)), hi))


def level_sizes(h, w, level):
    """sizes of the pyramid levels actually made: the loop stops once a level is smaller than the patch"""
    out = []
    for _ in range(level):
        if min(h, w) < PS:
            break
        h, w = h // 2, w // 2
        out.append((h, w))
    return out


def patch_workspace_bytes(b, h, w, level):
    """the documented workspace of balf_extract_patches_batch: 256 + every level made, [B,h,w] fp32, rounded up to 256"""
    return 256 + sum((b * hh * ww * 4 + 255) // 256 * 256 for hh, ww in level_sizes(h, w, level))


def _resize_axis(n_in, n_out):
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0


def pyrdown_f64(img):
    """5x5 binomial blur ([1,4,6,4,1]^2 / 256, reflect border), then bilinear resampling to (h//2, w//2),
    align_corners=False"""
    h, w = img.shape
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    p = np.pad(img, 2, mode="reflect")
    v = sum(k[d] * p[d:d + h, :] for d in range(5))
    blur = sum(k[d] * v[:, d:d + w] for d in range(5))
    y0, y1, ly = _resize_axis(h, h // 2)
    x0, x1, lx = _resize_axis(w, w // 2)
    top = blur[y0][:, x0] * (1.0 - lx) + blur[y0][:, x1] * lx
    bot = blur[y1][:, x0] * (1.0 - lx) + blur[y1][:, x1] * lx
    return top * (1.0 - ly)[:, None] + bot * ly[:, None]


def extract_patches_f64(gray_u8, xy, scale):
    """The algorithm oracle.extract_patches documents, in float64: uint8 / 255, pyramid level, LAF scale and centre
    carried to the level, the (2i + 1)/PS - 1 grid, grid_sample(bilinear, border, align_corners=False).
    gray_u8 [H,W] uint8, xy [N,2] fp32 (x, y) -> [N,32,32] float64."""
    img = np.asarray(gray_u8, np.float64) / 255.0
    xy = np.asarray(xy, np.float64)
    scale = np.float64(np.float32(scale))                         # the library takes the scale as a float
    h0, w0 = img.shape
    cur = img
    for _ in level_sizes(h0, w0, level_f64(h0, w0, scale)):
        cur = pyrdown_f64(cur)
    hl, wl = cur.shape
    s_l = scale / float(min(h0 - 1, w0 - 1)) * float(min(hl - 1, wl - 1))
    x_l = xy[:, 0] / (w0 - 1) * (wl - 1)
    y_l = xy[:, 1] / (h0 - 1) * (hl - 1)
    base = (2.0 * np.arange(PS, dtype=np.float64) + 1.0) / PS - 1.0
    gx = 2.0 * (s_l * base[None, :] + x_l[:, None]) / (wl - 1) - 1.0          # [N,PS]
    gy = 2.0 * (s_l * base[None, :] + y_l[:, None]) / (hl - 1) - 1.0
    fx = np.clip(((gx + 1.0) * wl - 1.0) * 0.5, 0.0, wl - 1.0)
    fy = np.clip(((gy + 1.0) * hl - 1.0) * 0.5, 0.0, hl - 1.0)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    lx, ly = fx - x0, fy - y0
    x1, y1 = np.minimum(x0 + 1, wl - 1), np.minimum(y0 + 1, hl - 1)
    yy0, yy1 = y0[:, :, None], y1[:, :, None]
    xx0, xx1 = x0[:, None, :], x1[:, None, :]
    wy, wx = ly[:, :, None], lx[:, None, :]
    return ((1.0 - wy) * ((1.0 - wx) * cur[yy0, xx0] + wx * cur[yy0, xx1])
            + wy * ((1.0 - wx) * cur[yy1, xx0] + wx * cur[yy1, xx1]))


_B32 = np.float32(32.0)
# (H, W, scale, what it exercises)
PATCH_CASES = [
    (160, 200, 300.0, "level 4 asked, 3 made"),
    (128, 128, 130.0, "three levels made"),
    (131, 203, 130.0, "odd sizes through three levels"),
    (64, 200, 130.0, "clamped by min(H,W)/32 - 1"),
    (20, 50, 60.0, "below the patch size, level 0 from uint8"),
    (31, 33, 60.0, "below the patch size"),
    (2, 2, 3.0, "the 2x2 minimum"),
    (96, 96, 16.0, "exact power of two"),
    (96, 96, 32.0, "exact power of two"),
    (96, 96, 64.0, "exact power of two"),
    (96, 96, float(np.nextafter(_B32, np.float32(0.0))), "just below a level switch"),
    (96, 96, float(np.nextafter(_B32, np.float32(64.0))), "just above a level switch"),
]
PATCH_POINTS = 64
# Largest |fp32 oracle.extract_patches - extract_patches_f64| over PATCH_CASES, measured on the CPU (both are references;
# tests/test_descriptor_edges_host.py re-measures it and asserts it is not above this record).  The GPU gets
# PATCH_GPU_FACTOR times this against the fp64 reference: its fp32 coordinate arithmetic is ordered differently from
# torch's, and the term scales with coordinate ulp x local contrast.
PATCH_F32_ORACLE_VS_F64 = 1.27e-5          # measured 1.262e-5 (96x96, scale 16: level 0, uint8 noise)
PATCH_GPU_FACTOR = 4.0


def patch_image(h, w):
    """uint8 noise, unsmoothed: the largest local contrast a coordinate error can meet"""
    return np.random.default_rng(7 * h + w).integers(0, 256, size=(h, w), dtype=np.uint8)


def patch_points(h, w, n=PATCH_POINTS):
    """the four corners, half-pixel positions, two points outside the image (border clamp), random interior points"""
    rng = np.random.default_rng(h * 1000 + w)
    xy = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], axis=1).astype(np.float32)
    xy[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    xy[4:8] = [[0.5, 0.5], [w - 1.5, h - 1.5], [(w - 1) // 2 + 0.5, (h - 1) // 2 + 0.5], [0.5, h - 1.5]]
    xy[8:10] = [[-5.0, -5.0], [w + 3.0, h + 7.0]]
    return xy


def gray_formula(rgb):
    """PIL's convert('L') in integers (tests/test_demo_gpu.py pins it to PIL itself)"""
    r, g, b = (rgb[..., c].astype(np.uint32) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)
