"""The split-f16 forward at the sizes where the way the persistent branch kernels hand groups to their waves can go wrong.
Stages 1-2 start 2048 waves (1024 wave pairs); the lower and the upper half of a workgroup's waves walk two ranges of the
groups, [0, split) and [split, total) (stage1_f16.h: BALF_S1_SHARE0, stage2_f16.h):

  64 x 64    64 stage-1 groups per image (16 at stage 2): most waves have no group at all and must leave at once, some
             workgroups have work for one half of their waves only, a range is shorter than one round; stage 4 is a single
             workgroup;
  128 x 192  384 groups per image: no multiple of any stride, the last round of either range is partial;
  192 x 320  960 groups per image, 2880 for the batch of three: more than one round of the lower waves, the second partial.

Which wave computes a group, and when, must change no bit: the outputs stay within the tolerance of the exact-fp32 kernels,
identical from run to run, and identical for an image alone and inside a batch (whose ranges split elsewhere).

Tolerances: score map 2e-5 against the fp32 kernels -- the bound tests/test_forward_gpu.py holds the split path to under load
(measured 4-6e-6); logits 1.5e-4, that file's tight gate on the split path's logits (measured 2e-5)."""
import numpy as np
import pytest
import torch

from balf_amd import arch
from balf_amd.utils import synth
from tests.golden import cases

pytestmark = pytest.mark.gpu
PROB_TOL = 2e-5
LOGIT_TOL = 1.5e-4
SHAPES = [(64, 64), (128, 192), (192, 320)]          # batches of 1 and 3 at each


def _load(precision):
    from balf_amd.model import get_model
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(cases.WEIGHT_SEED))
    m.precision = precision
    return m.eval().to("cuda:0")


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available()
    return _load("fp32"), _load("fp16")


def _inputs(kind, h, w):
    """Three images of exactly the padded size h x w (multiples of 64: nothing is padded)."""
    if kind == "float":
        return cases.forward_input(3, h, w, 1000 + h + w).to("cuda:0")
    rng = np.random.default_rng(2000 + h + w)
    return torch.from_numpy(rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)).to("cuda:0")


def _run(m, kind, x):
    with torch.inference_mode():
        out = m(x) if kind == "float" else m.forward_u8(x)
    return out["prob"], out["logits"]


@pytest.mark.parametrize("kind", ["float", "uint8"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_forward_is_right_deterministic_and_batch_invariant(models, hw, kind):
    m32, m16 = models
    h, w = hw
    x3 = _inputs(kind, h, w)
    ref_p, ref_l = _run(m32, kind, x3)                      # the exact-fp32 kernels, once, on the batch of three
    assert ref_p.shape == (3, h, w) and ref_l.shape == (3, 65, h // 8, w // 8)
    # batch of 3: tolerance, run to run
    p3, l3 = _run(m16, kind, x3)
    p3b, l3b = _run(m16, kind, x3)
    perr, lerr = (p3 - ref_p).abs().max().item(), (l3 - ref_l).abs().max().item()
    print(f"{h}x{w} {kind} B=3: prob err {perr:.3g} logit err {lerr:.3g}")
    assert perr < PROB_TOL and lerr < LOGIT_TOL
    assert torch.equal(p3, p3b) and torch.equal(l3, l3b)
    # batch of 1, every image: tolerance, run to run, and the image inside the batch of three
    for i in range(3):
        xi = x3[i:i + 1].contiguous()
        p1, l1 = _run(m16, kind, xi)
        p1b, l1b = _run(m16, kind, xi)
        perr, lerr = (p1 - ref_p[i:i + 1]).abs().max().item(), (l1 - ref_l[i:i + 1]).abs().max().item()
        print(f"{h}x{w} {kind} B=1 image {i}: prob err {perr:.3g} logit err {lerr:.3g}")
        assert perr < PROB_TOL and lerr < LOGIT_TOL
        assert torch.equal(p1, p1b) and torch.equal(l1, l1b)
        assert torch.equal(p1, p3[i:i + 1]) and torch.equal(l1, l3[i:i + 1]), (h, w, kind, i)
