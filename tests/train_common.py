"""What the reference modules of the training units (tests/*_train_common.py) share: the error measure of every gate, the
digest of the regenerated inputs, what a fixture records of a large result, and the slice geometry of the library's training
kernels restated (balf_amd/csrc/train_gemm.h: pixel_slices, and the three counts that a unit adds to it); the contents of the
``saved`` blocks as include/balf_hip.h lists them; and what the guard-band runs of tests/test_train_guard_gpu.py need: Guarded,
a buffer of an exact size between two bands of pattern, and GUARD_SHAPES, their shape table."""
import hashlib

import numpy as np
import torch


# ---- the slice geometry, restated ---------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


MAX_SLICES = 64                             # kMaxSlices: slabs of a weight gradient
MAX_COL_PARTS = 1024                        # what PC stays at or below: col_rows = rows / 16 once that exceeds 64


def pixel_slices(n):
    """train_gemm.h: pixel_slices(N) -> (rows, S, col_rows, PC).  A weight gradient sums over the pixels in S slices of ``rows``
    pixels (256, or the multiple of 256 that keeps S at 64), a float64 column sum in PC workgroups of ``col_rows`` rows (64, or
    rows / 16, which keeps PC at 1024)."""
    rows = 256 * _ceil_div(_ceil_div(n, 256), MAX_SLICES)
    col_rows = rows // 16 if rows // 16 > 64 else 64
    return rows, _ceil_div(n, rows), col_rows, _ceil_div(n, col_rows)


def last_part(n, size):
    """The length of the last of the ceil(n / size) parts of ``n`` rows: in 1..size."""
    return n - (_ceil_div(n, size) - 1) * size


def head_row_partials(n):
    """head_train.hip: P, the partials per channel of the row kernels (1024 pixels per workgroup), channel-major [65][P]."""
    return _ceil_div(n, 1024)


def rcab_image_blocks(hw):
    """rcab_train.hip: (img_rows, PI), the PI row blocks of img_rows rows of ONE image of hw pixels in img_sum_kernel: 64 rows, or
    what keeps PI at 1024."""
    per = _ceil_div(hw, 1024)
    img_rows = per if per > 64 else 64
    return img_rows, _ceil_div(hw, img_rows)


def gmlp_mix_groups(n):
    """gmlp_train.hip: (groups, gpw, PW): the groups of 64 tokens, the groups per workgroup of mix_bwd_kernel (at most 256
    workgroups) and the workgroups."""
    groups = n // 64
    gpw = _ceil_div(groups, 256)
    return groups, gpw, _ceil_div(groups, gpw)


def linrelu_workspace_bytes(n, c_in):
    """linrelu_train.hip: make_layout: gm [N, 2c] float32, the column partials [PC, 2c] float64, the slabs [S, 2c, c] float32, each
    rounded up to 256 bytes."""
    _, s, _, pc = pixel_slices(n)
    al = lambda b: _ceil_div(b, 256) * 256                      # noqa: E731
    return al(n * 2 * c_in * 4) + al(pc * 2 * c_in * 8) + al(s * 2 * c_in * c_in * 4)


# The smallest shapes that reach the upper regimes of that geometry and meet each unit's shape rules: (B, Hc, Wc), for linrelu
# (N, c_in).  The GPU sweeps append them to their own; tests/test_train_geometry_host.py asserts what each is there for.
LARGE_SHAPES = {
    "head": ((1, 129, 131), (1, 257, 257)),
    "rcab": ((1, 129, 131), (2, 257, 257)),
    "gmlp": ((1, 8, 2056), (2, 216, 152)),
    "linrelu": ((16899, 128), (65536, 128), (65537, 32), (65537, 128)),
}


# ---- what a ``saved`` block holds, as include/balf_hip.h lists it -----------------------------------------------------------------
def head_saved_contents(n):
    """balf_head_train_forward: a [N,256], z channel-major [65,N], (mu, r) [2,65] float64 -> (name, bytes) per listed item."""
    return (("a", n * 256 * 4), ("z", 65 * n * 4), ("mu, r", 2 * 65 * 8))


def rcab_saved_contents(b, hc, wc):
    """balf_rcab_train_forward: n, a, t [N,256], (mean, rstd) per pixel, and per image m [256], e [64], s [256] as float64 and s
    once more as float32."""
    n = b * hc * wc
    return (("n", n * 1024), ("a", n * 1024), ("t", n * 1024), ("mean, rstd", n * 8), ("m", b * 256 * 8), ("e", b * 64 * 8),
            ("s", b * 256 * 8), ("s as float32", b * 256 * 4))


def gmlp_saved_contents(b, hc, wc):
    """balf_gmlp_train_forward: n0 [N,256], h0, gelu(h0), cat [N,512], the (mean, rstd) [N,2] of the five LayerNorms, and per branch
    nb [N,256], hb, gelu(hb) [N,512], cn, mix + 1 and a (mix + 1) [N,256]."""
    n = b * hc * wc
    branch = (("nb", n * 1024), ("hb", n * 2048), ("gelu(hb)", n * 2048), ("cn", n * 1024), ("mix + 1", n * 1024),
              ("a (mix + 1)", n * 1024))
    return ((("n0", n * 1024), ("h0", n * 2048), ("gelu(h0)", n * 2048), ("cat", n * 2048))
            + tuple((f"(mean, rstd) of LN {i}", n * 8) for i in range(5))
            + tuple((f"{which} {k}", v) for which in ("grid", "block") for k, v in branch))


SAVED_REGION_ALIGN = 256                    # WorkspaceCursor rounds every region up to this


def saved_bounds(contents):
    """-> (low, high): a ``*_saved_bytes`` lies in [sum of the listed items, that + 256 per item]."""
    low = sum(v for _, v in contents)
    return low, low + SAVED_REGION_ALIGN * len(contents)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------
GUARD = 1 << 20                             # bytes of pattern on either side of a guarded buffer
GUARD_PAT = 0xA5
NAN_BYTE = 0xFF                             # a buffer of these bytes reads as NaN in float32 and in float64


class Guarded:
    """``nbytes`` usable bytes between two guard bands of ONE uint8 allocation (tests/test_guard_gpu.py: Guarded); .ptr is what
    the library gets.  ``offset``: the usable region starts that many bytes behind a 256-byte boundary (the lower band grows by
    them), for the paths that look at a pointer's alignment.  ``fill``: the byte the usable region starts with (None: the
    pattern).  A stray store of up to GUARD bytes on either side lands in a band of the same allocation and is reported."""

    def __init__(self, nbytes, fill=None, offset=0, device="cuda:0"):
        self.n, self.lo = int(nbytes), GUARD + int(offset)
        self.full = torch.full((self.lo + self.n + GUARD,), GUARD_PAT, dtype=torch.uint8, device=device)
        self.ptr = self.full.data_ptr() + self.lo
        assert self.ptr % 256 == offset % 256
        if fill is not None:
            self.fill(fill)

    @classmethod
    def of(cls, t, offset=0):
        """A guarded copy of tensor ``t``, of exactly its bytes."""
        g = cls(t.numel() * t.element_size(), offset=offset, device=t.device)
        g.load(t)
        return g

    def bytes(self):
        return self.full[self.lo:self.lo + self.n]

    def fill(self, byte):
        self.bytes().fill_(byte)

    def load(self, t):
        self.bytes().copy_(t.contiguous().reshape(-1).view(torch.uint8))

    def view(self, dtype, shape):
        return self.bytes().view(dtype).view(shape)

    def holds(self, byte):
        """Every usable byte is ``byte``: nothing was written since fill(byte)."""
        return bool((self.bytes() == byte).all())

    def intact(self):
        return bool((self.full[:self.lo] == GUARD_PAT).all()) and bool((self.full[self.lo + self.n:] == GUARD_PAT).all())


# ---- the shapes of the guard-band runs (tests/test_train_guard_gpu.py) ----------------------------------------------------------
def geometry(n, hw=None, c_in=None):
    """The figures of N pixels that the rows of GUARD_SHAPES quote: the slice geometry, the 64-row GEMM tiles, and what a unit
    adds (``hw``: the pixels of one image)."""
    rows, s, col_rows, pc = pixel_slices(n)
    g = dict(N=n, rows=rows, S=s, last_slice=last_part(n, rows), col_rows=col_rows, PC=pc, last_block=last_part(n, col_rows),
             tiles=_ceil_div(n, 64), last_tile=last_part(n, 64), P=head_row_partials(n))
    if hw is not None:
        g["img_rows"], g["PI"] = rcab_image_blocks(hw)
        g["last_img_block"] = last_part(hw, g["img_rows"])
    if n % 64 == 0:
        g["groups"], g["gpw"], g["PW"] = gmlp_mix_groups(n)
    return g


# unit -> ((shape, what it reaches as figures of geometry()), ...): (B, Hc, Wc), for linrelu (N, c_in).  The smallest shapes that
# reach each place where a size or a ragged edge of the training kernels changes; check_guard_shapes() holds every figure
# against pixel_slices and its companions.
_UPPER = {
    16899: dict(rows=512, S=34, last_slice=3, PC=265, last_block=3, last_tile=3, P=17),
    65536: dict(rows=1024, S=64, last_slice=1024, col_rows=64, PC=1024, last_block=64, last_tile=64),
    65537: dict(rows=1280, S=52, last_slice=257, col_rows=80, PC=820, last_block=17, last_tile=1),
    66049: dict(rows=1280, S=52, last_slice=769, col_rows=80, PC=826, last_block=49, last_tile=1, P=65),
}
GUARD_SHAPES = {
    "head": (
        ((1, 1, 2), dict(N=2, S=1, PC=1, tiles=1, last_tile=2, P=1)),                       # the minimum: two rows of one tile
        ((1, 5, 13), dict(N=65, S=1, PC=2, last_block=1, tiles=2, last_tile=1)),            # one row past a 64-row tile; zT 65 x 65
        ((1, 1, 257), dict(N=257, S=2, last_slice=1, PC=5, last_block=1, last_tile=1)),     # two slabs, the second of one row
        ((1, 129, 131), _UPPER[16899]),                                                     # the middle regime (LARGE_SHAPES)
        ((1, 257, 257), _UPPER[66049]),                                                     # the upper regime, P = 65
    ),
    "rcab": (
        ((2, 1, 1), dict(N=2, S=1, PC=1, PI=1, last_img_block=1)),                          # one pixel per image
        ((1, 5, 13), dict(N=65, tiles=2, last_tile=1, PI=2, last_img_block=1)),             # one row past a tile and an image block
        ((2, 7, 9), dict(N=126, tiles=2, last_tile=62, PI=1, last_img_block=63)),           # image 1 begins at row 63 of tile 0
        ((1, 1, 257), dict(N=257, S=2, last_slice=1, PC=5, PI=5, last_img_block=1)),        # two slabs, five image blocks
        ((1, 129, 131), dict(_UPPER[16899], PI=265, last_img_block=3)),
        ((2, 257, 257), dict(N=132098, rows=2304, S=58, last_slice=770, col_rows=144, PC=918, last_block=50, last_tile=2,
                             img_rows=65, PI=1017, last_img_block=9)),                      # the upper regime, two images
    ),
    "gmlp": (
        ((1, 8, 8), dict(N=64, S=1, PC=1, tiles=1, groups=1, PW=1)),                        # one group, one tile
        ((2, 8, 16), dict(N=256, S=1, last_slice=256, PC=4, groups=4, gpw=1, PW=4)),        # the last N of one slab; two images
        ((1, 8, 40), dict(N=320, S=2, last_slice=64, PC=5, groups=5)),                      # two slabs, the second of 64 rows
        ((1, 8, 2056), dict(N=16448, rows=512, S=33, last_slice=64, PC=257, groups=257, gpw=2, PW=129)),
        ((2, 216, 152), dict(N=65664, rows=1280, S=52, last_slice=384, col_rows=80, PC=821, last_block=64, groups=1026, gpw=5,
                             PW=206)),
    ),
    "linrelu": (
        ((1, 128), dict(N=1, S=1, PC=1, last_tile=1)),                                      # one row
        ((63, 128), dict(N=63, tiles=1, last_tile=63)),                                     # one row short of a tile
        ((65, 32), dict(N=65, tiles=2, last_tile=1, PC=2, last_block=1)),                   # one row past it, the narrowest width
        ((257, 64), dict(N=257, S=2, last_slice=1, PC=5, last_block=1)),                    # two slabs, the middle width
        ((16899, 128), _UPPER[16899]),
        ((65536, 128), _UPPER[65536]),                                                      # both caps at once
        ((65537, 32), _UPPER[65537]),                                                       # the first N of the upper regime ...
        ((65537, 128), _UPPER[65537]),                                                      # ... at 16 and at 4 rows in flight
    ),
}


def guard_shape_pixels(unit, shape):
    return shape[0] if unit == "linrelu" else shape[0] * shape[1] * shape[2]


def check_guard_shapes():
    """Every figure quoted in GUARD_SHAPES is what the restated geometry gives, the two upper regimes are those of LARGE_SHAPES,
    and between them a unit's rows reach: one slab and several, a ragged last GEMM tile, and each of the three regimes."""
    for unit, table in GUARD_SHAPES.items():
        shapes = tuple(s for s, _ in table)
        assert set(LARGE_SHAPES[unit]) <= set(shapes), unit
        seen = []
        for shape, quoted in table:
            n = guard_shape_pixels(unit, shape)
            got = geometry(n, hw=None if unit == "linrelu" else shape[1] * shape[2])
            assert {k: got[k] for k in quoted} == quoted, (unit, shape, {k: got[k] for k in quoted})
            seen.append(got)
        assert any(g["S"] == 1 for g in seen) and any(g["S"] == 2 for g in seen), unit
        assert unit == "gmlp" or any(g["last_tile"] < 64 for g in seen), unit      # (the gMLP's N is a multiple of 64)
        assert any(g["N"] <= 16384 for g in seen) and any(16384 < g["N"] <= 65536 for g in seen), unit
        assert any(g["N"] > 65536 for g in seen), unit


check_guard_shapes()


def to_device(case, device):
    """The tensors of a seeded case -- a tensor, a dict of them, tuples of either -- on ``device`` (None: as they are)."""
    if device is None:
        return case
    if isinstance(case, dict):
        return {k: to_device(v, device) for k, v in case.items()}
    if isinstance(case, (tuple, list)):
        return tuple(to_device(v, device) for v in case)
    return case.to(device)


def err(got, want64, scale):
    """max |got - want| / S, the measure of every gate."""
    want64 = torch.as_tensor(np.asarray(want64)).double() if not isinstance(want64, torch.Tensor) else want64.double()
    got = torch.as_tensor(np.asarray(got)) if not isinstance(got, torch.Tensor) else got.detach()
    got = got.double().to(want64.device)                # the difference is taken where the restatement lies
    return float((got.reshape(want64.shape) - want64).abs().max()) / scale


def composition_figures(what, composed, res, names, measure=err):
    """err(T) of the float32 torch-op composition's outputs ``composed`` (a unit's compose_f32 at the inputs of the case) in the
    scales of the restatement ``res``, printed next to the library's own: what any float32 implementation does at this shape.
    -> name -> figure."""
    figs = {k: measure(composed[k], res[k], res["S"][k]) for k in names if composed.get(k) is not None}
    print(what, "float32 composition:", " ".join(f"{k} {e:.2e}" for k, e in figs.items()))
    return figs


def inputs_digest(*tensors, keys=sorted):
    """SHA-256 over the float32 bytes of tensors, dicts (their values in the order ``keys(dict)``) and tuples of them: recorded
    next to the reference's results, so that a drift of a seeded generator or of synth.synthetic_state_dict -- which would
    silently pair new inputs with old results -- fails loudly instead."""
    h = hashlib.sha256()

    def feed(t):
        if isinstance(t, dict):
            for k in keys(t):
                feed(t[k])
        elif isinstance(t, (tuple, list)):
            for u in t:
                feed(u)
        else:
            h.update(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32)).tobytes())

    feed(tensors)
    return h.hexdigest()


def recorded_part(t, whole, every):
    """What a fixture records of a reference RESULT ``t``: all of it up to ``whole`` elements, else -- as a matrix of rows of
    its last axis -- rows 0..7 and every ``every``-th row.  A fixture must stay under 1 MB, and every output is checked whole
    against the float64 restatement anyway; d_T was taken on the whole results."""
    if t.numel() <= whole:
        return t
    rows = t.reshape(-1, t.shape[-1])
    return rows[sorted(set(range(8)) | set(range(0, rows.shape[0], every)))]


def recorded(fx, name, k, full, part):
    """-> (the reference's recorded float32 result, the same part of ``full``); ``part``: the module's recorded_part."""
    return torch.from_numpy(fx[f"{name}.{k}"]), part(full)
