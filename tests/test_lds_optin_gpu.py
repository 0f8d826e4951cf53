"""The dynamic-LDS opt-in (csrc/common.h: balf_allow_dynamic_lds) along its grow path, in ONE process: a kernel whose LDS size
depends on an argument is run below 48 KiB (no opt-in), then past it (the first opt-in), then at a larger size (the opt-in
must be renewed: the driver holds the last size granted), then small again (the record must not shrink).  Every result is
compared bit for bit with its restatement, so a launch that was refused or ran with too little LDS fails here."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import test_multiscale_edges_gpu as ME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from balf_amd import _lib
    assert _lib.lib().balf_device_check() == 0, "not a gfx950 device"
    return torch.device("cuda:0")


def test_topk_select_small_large_larger_small(dev):
    """balf_nms_topk on a 128 x 128 map: the select kernel takes next_pow2(K) * 8 + 1056 bytes of LDS, 2 KiB at K = 100, 65 KiB
    at K = 5000, 129 KiB at K = 10000."""
    from balf_amd import ops
    from oracle import c_oracle
    h = w = 128
    score = np.random.default_rng(48).random((h, w), dtype=np.float32)
    t = torch.from_numpy(score).to(dev).unsqueeze(0)
    for k in (100, 5000, 10000, 100):
        idx, sc, cnt = ops.nms_topk(t, 0, 0, h, w, 0, 3, k)
        idx, sc, n = idx.cpu().numpy()[0], sc.cpu().numpy()[0], int(cnt.cpu().numpy()[0])
        ri, rs, _ = c_oracle.nms_topk(score, 0, 3, k)
        ri, rs = O.canonical_order(ri.astype(np.int64), rs)
        assert n == ri.size, k
        assert np.array_equal(idx[:n], ri.astype(np.int32)), k
        assert np.array_equal(sc[:n].view(np.uint32), rs.view(np.uint32)), k
        assert np.all(idx[n:] == -1), k


def test_merge_small_large_larger_small(dev):
    """balf_multiscale_merge of three levels: the kernel sorts next_pow2(min(3 K_max, 16384)) keys of 8 bytes in LDS: 32 KiB at
    K_max = 1024, 64 KiB at K_max = 1366 (4098 keys: the smallest size past 48 KiB), 128 KiB at K_max = 3000."""
    rng = np.random.default_rng(49)
    for k_max in (1024, 1366, 3000, 1024):
        count = np.array([[k_max, 5], [k_max // 2, 0], [k_max - 1, 3]], np.int32)
        idx, sc = ME._level_lists(rng, count, k_max, ME.WIDTHS3, ME.HEIGHTS3)
        _, gc, _ = ME._merge_check(idx, sc, count, ME.WIDTHS3, ME._diag_hms(3), 2000, False)
        assert list(gc) == [min(2000, int(count[:, 0].sum())), 8], k_max
