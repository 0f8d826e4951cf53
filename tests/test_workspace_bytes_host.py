"""Every size query of the library against the bytes it returned before the layouts moved onto one cursor (no GPU).

Each ``*_workspace_bytes`` / ``*_saved_bytes`` export (and ``balf_forward_micro_batch``, which comes out of the same plan) is
called over the table below and must return what tests/golden/workspace_bytes.json holds.  The fixture was recorded from a
build of the commit BEFORE the change under test, never from the code under test:

    BALF_HIP_LIB=<that build's libbalf_hip.so> python tests/test_workspace_bytes_host.py --record

with BALF_MB_MPIXELS and BALF_HN_CHUNK unset (both change the sizes and are read once per process).  A caller's workspace is
allocated from these numbers, and the kernels' pointers come from the same layout function, so a size that moves here is a
layout that moved.  After a change that is MEANT to move a layout, record again from the commit before it plus that change
alone, and say so in the commit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest

from balf_amd import _lib

GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
TUNING_ENV = ("BALF_MB_MPIXELS", "BALF_HN_CHUNK")

BS = (1, 63, 64, 65)                        # B * 4 bytes crosses a 256-byte slice between 64 and 65
ODD, VGA, HD = (37, 53), (480, 640), (1080, 1920)
GREEDY, WINDOW = _lib.VAL_LEG_GREEDY, _lib.VAL_LEG_WINDOW

_maps = [(b, *ODD) for b in BS] + [(1, *VGA), (8, *VGA), (2, *HD), (32, 1088, 1920)]
# the forward's micro-batch is 2^25 padded pixels: 8192 images of 64 x 64, 16 of 1088 x 1920
_forward = [(b, 64, 64) for b in (1, 8191, 8192, 8193)] + [(b, 1088, 1920) for b in (1, 15, 16, 17, 32)] + [(3, 128, 192), (1, 5760, 5760)]
_train_dims = [(1, 1, 2), (63, 1, 5), (64, 1, 1), (65, 1, 1), (3, 5, 7), (4, 24, 24), (16, 64, 80)]
_train_n = [2, 63, 64, 65, 105, 2304, 81920]

# name -> (valid argument sets, one invalid set that must give 0)
TABLE = {
    "balf_forward_workspace_bytes": (_forward, (1, 100, 64)),
    "balf_forward_micro_batch": (_forward, (0, 64, 64)),
    # (B, H, W, K)
    "balf_nms_topk_workspace_bytes": ([m + (k,) for m in _maps for k in (1, 1000)], (0, 37, 53, 10)),
    # ... a map narrower and lower than one 64 x 32 tile, one just past a tile, K that does not enter the layout
    "balf_greedy_nms_workspace_bytes": ([m + (k,) for m in _maps + [(1, 5, 7), (3, 31, 63), (2, 33, 65), (65, 1, 1)] for k in (1, 512)],
                                        (1, 37, 0, 10)),
    "balf_hardnet_workspace_bytes": ([(n,) for n in (1, 8, 4095, 4096, 4097, 10000)], (0,)),
    # (B, H, W, scale): the level is floor(log2(scale / 16)) clamped to [0, min(H, W) / 32 - 1]: scale 8 and 16 give no level, 32
    # one, 128 three; 1e4 asks for nine and the 480 x 640 loop stops after four (30 rows < 32); 37 x 53 never has one
    "balf_extract_patches_batch_workspace_bytes": (
        [(b, h, w, s) for b in (1, 63) for (h, w) in (VGA, (101, 135)) for s in (8.0, 16.0, 32.0, 128.0, 1e4)]
        + [(65, *ODD, 64.0), (2, *HD, 64.0), (1, *HD, 1e4), (64, 64, 64, 32.0), (1, 32, 2000, 1e4)], (1, 480, 640, 0.0)),
    "balf_extract_patches_workspace_bytes": ([(h, w, s) for (h, w) in (VGA, HD, ODD, (101, 135)) for s in (8.0, 32.0, 128.0, 1e4)],
                                             (480, 0, 32.0)),
    # (pairs, k1, k2): k1 != k2, and pairs * k * 8 that is no multiple of 256 (3 * 5 * 8 = 120, 999 * 8 = 7992)
    "balf_match_smnn_batch_workspace_bytes": ([(1, 1, 1), (1, 32, 32), (3, 5, 7), (1, 100, 37), (80, 1000, 999)]
                                              + [(p, 33, 31) for p in BS], (0, 5, 5)),
    "balf_match_smnn_workspace_bytes": ([(1, 1), (32, 32), (100, 37), (999, 1000), (16384, 1)], (5, 0)),
    # (ns, nd, max_edges)
    "balf_repeatability_workspace_bytes": ([(1, 1, 1), (37, 53, 100), (63, 65, 64), (1000, 999, 5000), (16384, 16384, 1)], (0, 5, 5)),
    # (P, ns_max, nd_max, max_edges)
    "balf_repeatability_batch_workspace_bytes": ([(p, 37, 53, 100) for p in BS] + [(1, 0, 0, 1), (64, 1000, 999, 5000)], (1, 5, 5, 0)),
    # (P, h_src, w_src, h_dst, w_dst, leg, nms_size, K)
    "balf_val_points_workspace_bytes": (
        [(p, *ODD, 53, 37, leg, 3, 25) for p in BS for leg in (GREEDY, WINDOW)]
        + [(2, *VGA, *VGA, GREEDY, 15, 1000), (2, *VGA, 240, 320, WINDOW, 15, 1000), (1, *HD, *HD, GREEDY, 15, 5000),
           (1, *HD, *HD, WINDOW, 9, 16384), (3, 5, 7, 9, 4, GREEDY, 0, 10), (3, 5, 7, 9, 4, WINDOW, 1, 10)],
        (1, *ODD, *ODD, 2, 3, 25)),
    # (P, ns_max, nd_max, keep_k_points)
    "balf_resize_repeatability_batch_workspace_bytes": ([(p, 37, 53, 25) for p in BS] + [(1, 0, 0, 1), (64, 1000, 999, 1000)],
                                                        (1, 5, 5, 0)),
    # (P, patch)
    "balf_synth_pairs_workspace_bytes": ([(p, 37) for p in BS] + [(1, 1), (1, 512), (65, 512), (3, 16384)], (0, 512)),
    # (B, Hc, Wc)
    "balf_detector_loss_workspace_bytes": ([(b, 5, 7) for b in BS] + [(1, 1, 1), (64, 32, 32), (32, 136, 240)], (0, 5, 7)),
    "balf_head_train_workspace_bytes": ([(n,) for n in _train_n], (1,)),
    "balf_head_train_saved_bytes": ([(n,) for n in _train_n], (1,)),
    "balf_rcab_train_workspace_bytes": (_train_dims, (1, 1, 1)),
    "balf_rcab_train_saved_bytes": (_train_dims, (1, 1, 1)),
    "balf_gmlp_train_workspace_bytes": ([(b, 8, 8) for b in BS] + [(1, 8, 16), (4, 24, 24), (16, 64, 80)], (1, 7, 8)),
    "balf_gmlp_train_saved_bytes": ([(b, 8, 8) for b in BS] + [(1, 8, 16), (4, 24, 24), (16, 64, 80)], (1, 7, 8)),
    # (N, c_in)
    "balf_linrelu_train_workspace_bytes": ([(n, c) for n in (1, 63, 65, 2304) for c in (32, 64, 128)], (5, 48)),
}


def size_exports():
    return sorted(n for n in _lib.PROTOTYPES if n.endswith(("_workspace_bytes", "_saved_bytes"))) + ["balf_forward_micro_batch"]


def key(args):
    return " ".join(repr(a) for a in args)


def query(lib):
    assert not [e for e in TUNING_ENV if e in os.environ], f"unset {TUNING_ENV}: they change the sizes"
    return {name: {key(a): int(getattr(lib, name)(*a)) for a in valid + [invalid]} for name, (valid, invalid) in TABLE.items()}


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_every_size_export(golden):
    assert sorted(TABLE) == sorted(size_exports()) == sorted(golden)
    for name, (valid, invalid) in TABLE.items():
        assert sorted(golden[name]) == sorted(key(a) for a in valid + [invalid]), name
        # the recorded table itself: every valid set had a size, the invalid one none
        assert all(golden[name][key(a)] > 0 for a in valid), name
        assert golden[name][key(invalid)] == 0, name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_size_query_returns_the_recorded_bytes(lib, golden, name):
    if [e for e in TUNING_ENV if e in os.environ] and name in ("balf_forward_workspace_bytes", "balf_forward_micro_batch",
                                                                "balf_hardnet_workspace_bytes"):
        pytest.skip(f"one of {TUNING_ENV} is set: the recorded sizes are those of the defaults")
    valid, invalid = TABLE[name]
    got = {key(a): int(getattr(lib, name)(*a)) for a in valid + [invalid]}
    assert got == golden[name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    print(f"recording from {_lib.LIB_PATH}")
    with open(GOLDEN, "w") as f:
        json.dump(query(_lib.lib()), f, indent=0, sort_keys=True)
        f.write("\n")
