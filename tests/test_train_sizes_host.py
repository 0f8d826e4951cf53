"""The size queries of the four training units against literals: the workspace and saved layouts are part of what a caller
allocates, and all of them hang on the one pixel-slice geometry of train_gemm.h (pixel_slices).  The literals were recorded
from the library as it stood before the units' layouts were put onto that one function.  N = 2, 64 and 256 are one slice, 257
a ragged second one, 16384 the last N with 256 pixels per slice, 16385 the first with more (and 5 x 29 x 113 pixels: nothing
divides), 17408 = 128 x 136 the edge case of the GPU suites, 81920 a training batch, 2^24 the largest N.  16448, 16899, 65536,
65537, 65664, 66049 and 132098 are the pixel counts at which the GPU sweeps cross the thresholds of that geometry
(tests/test_train_geometry_host.py says what each reaches); their literals were recorded from the library as it stood when those
cases were added."""
import os

import pytest

from balf_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# N: (B, Hc, Wc), head (workspace, saved), rcab (workspace, saved), gmlp (workspace, saved; 0 where Hc or Wc is no multiple of 8),
# linrelu workspace at c_in = 32, 64, 128
SIZES = {
    2: ((1, 1, 2), (336128, 4096), (275968, 12032), (0, 0), (9216, 34816, 135168)),
    64: ((1, 8, 8), (415488, 83456), (402944, 202752), (1189888, 1509888), (25088, 66560, 198656)),
    256: ((1, 16, 16), (668160, 329984), (814592, 794112), (3186688, 6039552), (75776, 167936, 401408)),
    257: ((1, 1, 257), (1000448, 331520), (1084928, 797440), (0, 0), (84736, 202240, 535552)),
    16384: ((1, 128, 128), (42616320, 21038336), (51908096, 50468352), (203948032, 386531328), (4849664, 10747904, 25690112)),
    16385: ((5, 29, 113), (32431360, 21039872), (43810304, 50494208), (0, 0), (4596480, 9733632, 21629952)),
    17408: ((1, 128, 136), (34104064, 22353152), (46239232, 53622272), (180764672, 410689536), (4874240, 10305536, 22839296)),
    16448: ((1, 8, 2056), (32512000, 21120512), (43918848, 50665472), (171321344, 388041216), (4612608, 9765888, 21694464)),
    16899: ((1, 129, 131), (33436416, 21699840), (45153792, 52054784), (0, 0), (4740352, 10037760, 22303744)),
    65536: ((1, 256, 256), (107350272, 84149504), (157289984, 201856512), (612892672, 1546125312), (17825792, 36700160, 77594624)),
    65537: ((1, 1, 65537), (102990848, 84151040), (153280000, 201859840), (0, 0), (17623296, 36098560, 75604992)),
    65664: ((2, 216, 152), (103155712, 84313856), (153582592, 202256384), (599330816, 1549145088), (17656320, 36164608, 75737088)),
    66049: ((1, 257, 257), (103660544, 84808448), (154369536, 203436800), (0, 0), (17757440, 36366848, 76141568)),
    132098: ((2, 257, 257), (190695680, 169615360), (293673984, 406873344), (0, 0), (34762240, 70474752, 144750592)),
    81920: ((5, 128, 128), (128403968, 105186560), (191383040, 252341760), (747110400, 1932656640), (22020096, 45088768, 94371840)),
    1 << 24: ((4, 2048, 2048), (21582120192, 21541946624), (34389112832, 51673847808), (137514975232, 395808079872),
              (4296015872, 8593080320, 17190354944)),
}


@pytest.mark.parametrize("n", sorted(SIZES))
def test_size_queries_match_the_recorded_layouts(lib, n):
    dims, head, rcab, gmlp, linrelu = SIZES[n]
    assert dims[0] * dims[1] * dims[2] == n
    assert (lib.balf_head_train_workspace_bytes(n), lib.balf_head_train_saved_bytes(n)) == head
    assert (lib.balf_rcab_train_workspace_bytes(*dims), lib.balf_rcab_train_saved_bytes(*dims)) == rcab
    assert (lib.balf_gmlp_train_workspace_bytes(*dims), lib.balf_gmlp_train_saved_bytes(*dims)) == gmlp
    assert (gmlp == (0, 0)) == bool(dims[1] % 8 or dims[2] % 8)
    assert tuple(lib.balf_linrelu_train_workspace_bytes(n, c) for c in (32, 64, 128)) == linrelu
