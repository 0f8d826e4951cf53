"""The split-f16 guard retry (``guard.run_guarded``) in the two callers that run SEVERAL forwards before their one read and used
to repeat only on a flag found at that read: a later forward of the same run may already have consumed an earlier forward's flag
(repaired ``prob``, switched the checkpoint, warned) after the flagged score map went into the selection.  Whether that happens
depends on timing; the results must equal the fp32 model's either way."""
import warnings as W

import numpy as np
import pytest
import torch

from balf_amd import arch, multiscale
from balf_amd.model import get_model
from balf_amd.utils import train_utils
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def recipe():
    """(state dict, the saturated image [H,W,3], a calm image [H,W,3], the fp32 model): the checkpoint passes the load-time probes
    and leaves the f16 range on the saturated image (test_forward_gpu.py), 128 x 128."""
    from tests.test_forward_gpu import _scaled_checkpoint_and_images
    sd, bright = _scaled_checkpoint_and_images()

    def hwc(t):
        return t[0].permute(1, 2, 0).contiguous().numpy().astype(np.float64)
    return sd, hwc(bright), hwc(cases.forward_input(1, 128, 128, 3)), _model(sd, "fp32")


def _model(sd, precision="fp16"):
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(sd)
    m.precision = precision
    return m.eval().to(DEV)


def _fresh_fp16(sd, calm, monkeypatch):
    monkeypatch.delenv("BALF_FP16_STRICT", raising=False)
    monkeypatch.delenv("BALF_FP16_GUARD", raising=False)             # the default: lazy
    m = _model(sd)
    with W.catch_warnings():
        W.simplefilter("error")
        with torch.inference_mode():                                 # probes + an ordinary image: silent, split path
            m(torch.from_numpy(calm).permute(2, 0, 1)[None].float().to(DEV))
    assert m.effective_precision == "fp16"
    return m


def test_hsequences_chunk_with_a_flag_in_the_middle_equals_fp32(recipe, monkeypatch):
    """One sequence, batch_size=1: four separate forwards (calm source, calm, SATURATED, calm) before the one read."""
    sd, bright, calm, ref = recipe
    h = np.array([[1.0, 0.0, 4.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]])

    class Loader:
        sequences = ["s"]

        def get_sequence_data(self, i):
            return dict(im_src_RGB_norm=calm, h_dst_2_src=[h, h, h],
                        images_dst_RGB_norm=[np.ascontiguousarray(calm[:, ::-1]), bright, np.ascontiguousarray(calm[::-1])])

    want = train_utils.check_val_hsequences_repeatability(Loader(), ref, DEV, None, 0, num_points=25, batch_size=1)
    assert np.isfinite(want).all(), want
    m = _fresh_fp16(sd, calm, monkeypatch)
    with pytest.warns(RuntimeWarning, match="left the range of its f16 halves"):
        got = train_utils.check_val_hsequences_repeatability(Loader(), m, DEV, None, 0, num_points=25, batch_size=1)
    assert m.effective_precision == "fp32"
    for a, b in zip(got, want):
        assert np.array_equal(np.float64(a), np.float64(b)), (got, want)


def test_multiscale_extraction_of_a_flagged_image_equals_fp32(recipe, monkeypatch):
    """One forward per pyramid level; the level that is the image itself leaves the f16 range."""
    sd, bright, calm, ref = recipe
    want = multiscale.extract_multiscale_detections(bright, ref, DEV, num_points=200)
    assert want.shape[0] > 0
    m = _fresh_fp16(sd, calm, monkeypatch)
    with pytest.warns(RuntimeWarning, match="left the range of its f16 halves"):
        got = multiscale.extract_multiscale_detections(bright, m, DEV, num_points=200)
    assert m.effective_precision == "fp32"
    assert np.array_equal(got, want)
