"""launch() (balf_amd/_lib.py) puts the work on the CURRENT stream of the tensor's device: two wrappers called inside
``torch.cuda.stream(side)`` give the bits of their default-stream calls, and waiting for the side stream's event alone -- no
device-wide synchronisation -- is enough to read them."""
import pytest
import torch

from balf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_wrappers_run_on_the_side_stream_they_are_called_in():
    rgb = torch.tensor([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [13, 101, 200]]], dtype=torch.uint8, device=DEV)    # 2x2x3
    score = torch.rand((1, 8, 8), generator=torch.Generator().manual_seed(7)).to(DEV)
    want = (ops.rgb_to_gray_u8(rgb), ops.window_nms(score, 1, 3))
    torch.cuda.synchronize()
    want = tuple(t.cpu() for t in want)
    assert want[0].shape == (2, 2) and want[1].shape == (1, 8, 8) and int((want[1] > 0).sum()) > 0

    side = torch.cuda.Stream(DEV)
    assert side.cuda_stream != torch.cuda.current_stream(DEV).cuda_stream
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        got = (ops.rgb_to_gray_u8(rgb), ops.window_nms(score, 1, 3))
        done.record()                                               # on the side stream, behind the two launches
    done.synchronize()
    assert done.query()
    with torch.cuda.stream(side):                                   # (the copies go to the side stream too: nothing else is waited for)
        got = tuple(t.cpu() for t in got)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
