"""The slice geometry of the training kernels (balf_amd/csrc/train_gemm.h: pixel_slices, and the counts that head_train.hip,
rcab_train.hip and gmlp_train.hip add) as tests/train_common.py restates it:

* the restatement against the library: balf_linrelu_train_workspace_bytes(N, c) is a closed function of (S, PC), and must equal
  the mirror's at every N on both sides of each threshold of the geometry, for the three widths;
* the regime that each of train_common.LARGE_SHAPES is in the GPU sweeps for, as literals worked out by hand from the kernels'
  code: the comments of the GPU tests are claims that this file verifies.

The geometry has three regimes: N <= 16384 (rows 256, col_rows 64), N <= 65536 (rows 512 .. 1024, col_rows 64) and N >= 65537
(rows >= 1280, col_rows = rows / 16 >= 80, PC <= 1024)."""
import os

import pytest

from balf_amd import _lib
from tests import train_common as T


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def pixels(unit, shape):
    return shape[0] if unit == "linrelu" else shape[0] * shape[1] * shape[2]


CHUNK = 64 * 1024                           # N = 64 * 1024 * k is the last N with rows = 1024 k
THRESHOLDS = ([1, 2, 255, 256, 257, 16384, 16385, 17408, 65536, 65537, 81920]
              + [CHUNK * k + d for k in (2, 3, 5, 16, 100, 255) for d in (0, 1)] + [(1 << 24) - 1, 1 << 24])
SHAPE_NS = sorted({pixels(u, s) for u, shapes in T.LARGE_SHAPES.items() for s in shapes})


@pytest.mark.parametrize("n", sorted(set(THRESHOLDS + SHAPE_NS)))
def test_the_mirror_gives_the_library_s_linrelu_workspace(lib, n):
    for c in (32, 64, 128):
        assert lib.balf_linrelu_train_workspace_bytes(n, c) == T.linrelu_workspace_bytes(n, c), (n, c)


def test_the_mirror_at_the_literals_worked_out_by_hand():
    assert T.linrelu_workspace_bytes(17408, 128) == 22839296 and T.linrelu_workspace_bytes(81920, 32) == 22020096
    assert T.pixel_slices(1) == (256, 1, 64, 1) and T.pixel_slices(257) == (256, 2, 64, 5)
    assert T.pixel_slices(16384) == (256, 64, 64, 256) and T.pixel_slices(16385) == (512, 33, 64, 257)
    assert T.pixel_slices(17408) == (512, 34, 64, 272)
    assert T.pixel_slices(65536) == (1024, 64, 64, 1024) and T.pixel_slices(65537) == (1280, 52, 80, 820)
    assert T.pixel_slices(81920) == (1280, 64, 80, 1024)
    assert T.pixel_slices(1 << 24) == (262144, 64, 16384, 1024)


@pytest.mark.parametrize("n", sorted(set(THRESHOLDS + SHAPE_NS)))
def test_the_caps_hold(n):
    rows, s, col_rows, pc = T.pixel_slices(n)
    assert rows % 256 == 0 and 1 <= s <= T.MAX_SLICES and 1 <= pc <= T.MAX_COL_PARTS
    assert (s - 1) * rows < n <= s * rows and (pc - 1) * col_rows < n <= pc * col_rows
    assert col_rows == (64 if n <= 65536 else rows // 16)
    assert (rows > 256) == (n > 16384) and (col_rows > 64) == (n > 65536)      # the three regimes


# What pixel_slices gives at each N of LARGE_SHAPES: rows, S, the length of the last K slice (and, below, that length mod 16: the
# GEMM walks K in steps of 16), col_rows, PC, the rows of the last column block
SLICES = {
    16448: dict(rows=512, S=33, last_slice=64, col_rows=64, PC=257, last_block=64),
    16899: dict(rows=512, S=34, last_slice=3, col_rows=64, PC=265, last_block=3),
    65536: dict(rows=1024, S=64, last_slice=1024, col_rows=64, PC=1024, last_block=64),
    65537: dict(rows=1280, S=52, last_slice=257, col_rows=80, PC=820, last_block=17),
    65664: dict(rows=1280, S=52, last_slice=384, col_rows=80, PC=821, last_block=64),
    66049: dict(rows=1280, S=52, last_slice=769, col_rows=80, PC=826, last_block=49),
    132098: dict(rows=2304, S=58, last_slice=770, col_rows=144, PC=918, last_block=50),
}
LAST_SLICE_MOD_16 = {16448: 0, 16899: 3, 65536: 0, 65537: 1, 65664: 0, 66049: 1, 132098: 2}


@pytest.mark.parametrize("n", sorted(SLICES))
def test_slices_of_the_large_shapes(n):
    rows, s, col_rows, pc = T.pixel_slices(n)
    got = dict(rows=rows, S=s, last_slice=T.last_part(n, rows), col_rows=col_rows, PC=pc, last_block=T.last_part(n, col_rows))
    assert got == SLICES[n]
    assert got["last_slice"] % 16 == LAST_SLICE_MOD_16[n]


def test_every_large_shape_has_its_slices_asserted():
    assert SHAPE_NS == sorted(SLICES)
    # and between them the shapes reach: a slice of more than 256 rows that is short, and one whose length is no multiple of 16; a
    # column block of more than 64 rows that is short; both caps at once
    assert any(v["rows"] > 256 and v["last_slice"] < v["rows"] and v["last_slice"] % 16 for v in SLICES.values())
    assert any(v["col_rows"] > 64 and v["last_block"] < v["col_rows"] for v in SLICES.values())
    assert any(v["S"] == T.MAX_SLICES and v["PC"] == T.MAX_COL_PARTS for v in SLICES.values())


def test_head_shapes():
    """P = ceil(N / 1024) partials per channel, channel-major: wave_sum_strided takes a second trip from P = 65 on."""
    a, b = T.LARGE_SHAPES["head"]
    assert (pixels("head", a), pixels("head", b)) == (16899, 66049)
    assert T.head_row_partials(16899) == 17                     # one trip, 17 lanes
    assert T.head_row_partials(66049) == 65                     # exactly one lane (lane 0) takes a second trip
    assert T.last_part(66049, 1024) == 513                      # pixels of the last row workgroup
    assert max(T.head_row_partials(s[0] * s[1] * s[2]) for s in ((4, 32, 32), (2, 23, 37))) == 4       # what the sweep had reached


def test_rcab_shapes():
    """img_rows = max(64, ceil(hw / 1024)) rows per block of the sums over ONE image."""
    a, b = T.LARGE_SHAPES["rcab"]
    assert pixels("rcab", a) == 16899 and T.rcab_image_blocks(129 * 131) == (64, 265) and T.last_part(16899, 64) == 3
    assert pixels("rcab", b) == 132098 and b[0] == 2
    hw = b[1] * b[2]
    assert hw == 66049 and T.rcab_image_blocks(hw) == (65, 1017) and T.last_part(hw, 65) == 9
    assert T.rcab_image_blocks(65536) == (64, 1024)             # the last hw with 64 rows: one image must exceed 65536 pixels
    col_rows = T.pixel_slices(132098)[2]
    assert hw // col_rows == 458 and hw % col_rows == 97        # image 1 begins 97 rows into column block 458: dt_kernel's image index


def test_gmlp_shapes():
    """groups of 64 tokens, gpw = ceil(groups / 256) per workgroup of mix_bwd_kernel, PW workgroups."""
    a, b = T.LARGE_SHAPES["gmlp"]
    assert all(s[1] % 8 == 0 and s[2] % 8 == 0 for s in (a, b))
    assert pixels("gmlp", a) == 16448 and T.gmlp_mix_groups(16448) == (257, 2, 129) and T.last_part(257, 2) == 1
    assert (a[1] // 8, a[2] // 8) == (1, 257)                   # the grid map's regions: 1 x 257 pixels
    assert pixels("gmlp", b) == 65664 and T.gmlp_mix_groups(65664) == (1026, 5, 206) and T.last_part(1026, 5) == 1
    assert T.gmlp_mix_groups(17408) == (272, 2, 136) and T.last_part(272, 2) == 2         # what the sweep had reached: a full one


def test_linrelu_shapes():
    shapes = T.LARGE_SHAPES["linrelu"]
    assert shapes == ((16899, 128), (65536, 128), (65537, 32), (65537, 128))
    # relu_mask_colsum_kernel keeps kR = 1024 / c_out rows in flight: 16 at c_in = 32, 4 at c_in = 128; a last block of 17 rows is a
    # second trip of one row at 16 and a ragged fifth trip at 4
    assert [1024 // (2 * c) for _, c in shapes] == [4, 4, 16, 4]
    assert T.last_part(65537, 80) == 17 and 17 % 16 == 1 and 17 % 4 == 1
