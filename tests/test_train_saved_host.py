"""The ``saved`` sizes of the training units against what include/balf_hip.h says a block holds, and the shape table of the
guard-band runs (no GPU).

The header lists the contents of each ``saved`` block; tests/train_common.py restates each list as bytes per item.  The library
lays the items out with WorkspaceCursor, which rounds every region up to 256 bytes, so

    sum of the items  <=  *_saved_bytes  <=  sum of the items + 256 * (number of items)

A query that under-reports by a region, or a region that the header does not list, fails here before any kernel runs;
tests/test_train_guard_gpu.py then shows that the kernels stay inside exactly these sizes."""
import os

import pytest

from balf_amd import _lib
from tests import test_train_geometry_host as geo
from tests import test_train_sizes_host as sizes
from tests import train_common as T


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


NS = sorted(n for n in set(geo.THRESHOLDS + geo.SHAPE_NS) if n >= 2)       # N = 1 is outside the limits of all three units
# (B, Hc, Wc) with B > 1 as well: the per-image items of the RCAB; the shapes of the guard-band runs and of the recorded sizes
DIMS = sorted({s for unit in ("head", "rcab", "gmlp") for s, _ in T.GUARD_SHAPES[unit]}
              | {v[0] for v in sizes.SIZES.values()} | {(3, 1, 5), (7, 8, 8), (65535, 1, 1)})


def in_bounds(got, contents):
    low, high = T.saved_bounds(contents)
    return low <= got <= high


@pytest.mark.parametrize("n", NS)
def test_head_saved_bytes_hold_the_listed_contents(lib, n):
    got = lib.balf_head_train_saved_bytes(n)
    assert in_bounds(got, T.head_saved_contents(n)), (n, got, T.saved_bounds(T.head_saved_contents(n)))


@pytest.mark.parametrize("n", NS)
def test_rcab_saved_bytes_hold_the_listed_contents(lib, n):
    got = lib.balf_rcab_train_saved_bytes(1, 1, n)
    assert in_bounds(got, T.rcab_saved_contents(1, 1, n)), (n, got, T.saved_bounds(T.rcab_saved_contents(1, 1, n)))


@pytest.mark.parametrize("n", [n for n in NS if n % 64 == 0])
def test_gmlp_saved_bytes_hold_the_listed_contents(lib, n):
    dims = (1, 8, n // 8)                                       # Hc and Wc multiples of 8
    got = lib.balf_gmlp_train_saved_bytes(*dims)
    assert in_bounds(got, T.gmlp_saved_contents(*dims)), (n, got, T.saved_bounds(T.gmlp_saved_contents(*dims)))


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_saved_bytes_of_batched_shapes(lib, dims):
    n = dims[0] * dims[1] * dims[2]
    if n >= 2:
        assert in_bounds(lib.balf_head_train_saved_bytes(n), T.head_saved_contents(n)), dims
        assert in_bounds(lib.balf_rcab_train_saved_bytes(*dims), T.rcab_saved_contents(*dims)), dims
    if dims[1] % 8 == 0 and dims[2] % 8 == 0:
        assert in_bounds(lib.balf_gmlp_train_saved_bytes(*dims), T.gmlp_saved_contents(*dims)), dims


def test_the_bounds_tell_a_missing_region():
    """The restated lists themselves: the item counts, and two sums worked out by hand.  The padding that the library may add
    (under 256 bytes per region, and none behind a [N,256] float32 matrix) stays below the smallest item of a list -- the head's
    1040 bytes of statistics against at most 252 + 240 of padding, the RCAB's e [64] float64 against at most 248 -- so a size
    without any one item lies under the lower bound."""
    for contents in (T.head_saved_contents(2), T.rcab_saved_contents(1, 1, 2), T.gmlp_saved_contents(1, 8, 8)):
        low, high = T.saved_bounds(contents)
        assert all(v > 0 for _, v in contents) and high - low == 256 * len(contents)
    assert len(T.head_saved_contents(2)) == 3 and len(T.rcab_saved_contents(1, 1, 2)) == 8 and len(T.gmlp_saved_contents(1, 8, 8)) == 21
    # worked out by hand: N = 2 of the head is 2048 + 520 + 1040 bytes in three regions of 2048 + 768 + 1280
    assert T.saved_bounds(T.head_saved_contents(2)) == (3608, 4376)
    assert T.saved_bounds(T.gmlp_saved_contents(1, 8, 8))[0] == 64 * 23592 == 1509888


def test_the_guard_shape_table_quotes_the_restated_geometry():
    T.check_guard_shapes()
    for unit, large in T.LARGE_SHAPES.items():
        assert tuple(s for s, _ in T.GUARD_SHAPES[unit])[-len(large):] == large
