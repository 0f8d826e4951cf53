"""One autograd function per training unit serves every width (model.train_units): ``_GmlpTrain`` and ``_RcabTrain``
take the width from their parameters, in one process at 128, 256 and 128 again, with the bits of the direct
``ops.*_train_forward`` / ``_backward(..., channels=c)`` calls on the same tensors; and parameters of one width with an activation
of the other are refused by the metadata checks, before any launch.  The ``rcab_train`` / ``gmlp_train`` workspaces are shared
between the widths, so a stale, differently sized workspace is what could go wrong: the second run at 128 has the bits of the
first.  Shapes: two images (the per-image squeeze-excite mean, the grid map's regions of 1 x 2 pixels) and an odd row count."""
import pytest
import torch

from balf_amd import ops
from balf_amd._lib import BalfHipError
from balf_amd.model.mixer_train import _GmlpTrain
from balf_amd.model.tail_train import _RcabTrain
from tests import gmlp_train_common as G
from tests import rcab_train_common as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GMLP_SHAPE, RCAB_SHAPE = (2, 8, 16), (2, 3, 5)
ORDER = (128, 256, 128)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def all_bits_equal(got, want):
    return len(got) == len(want) and all(bits_equal(a, b) for a, b in zip(got, want))


def leaf(t):
    return t.detach().requires_grad_()          # the same storage: the function and the direct call read the same tensors


def gmlp_by_function(x0, p, g):
    """-> [y, dx0, the 26 gradients]"""
    x, leaves = leaf(x0), [leaf(p[k]) for k in G.PARAMS]
    y = _GmlpTrain.apply(x, *leaves)
    y.backward(g)
    return [y.detach(), x.grad] + [t.grad for t in leaves]


def gmlp_direct(x0, p, g, c):
    params = [p[k] for k in G.PARAMS]
    f = ops.gmlp_train_forward(x0, params, channels=c)
    b = ops.gmlp_train_backward(g, x0, params, f.saved, want_dx0=True, channels=c)
    return [f.y, b.dx0] + list(b.grads)


def rcab_by_function(y, r, p, g):
    """-> [x2, dy, dr, the ten gradients]"""
    yy, rr, leaves = leaf(y), leaf(r), [leaf(p[k]) for k in R.PARAMS]
    x2 = _RcabTrain.apply(yy, rr, *leaves)
    x2.backward(g)
    return [x2.detach(), yy.grad, rr.grad] + [t.grad for t in leaves]


def rcab_direct(y, r, p, g, c):
    f = ops.rcab_train_forward(y, r, [p[k] for k in R.PARAMS], channels=c)
    b = ops.rcab_train_backward(g, y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], f.saved, want_dy=True, channels=c)
    return [f.x2, b.dy, g] + list(b[:10])       # the gradient of r = y + the long shortcut is dx2 itself


@pytest.fixture(scope="module")
def cases():
    """width -> (the gMLP sweep case, the RCAB sweep case), from the merged generators."""
    return {c: (G.sweep_case(GMLP_SHAPE, 31, device=DEV, c=c), R.sweep_case(RCAB_SHAPE, 37, device=DEV, c=c)) for c in (128, 256)}


@pytest.fixture(scope="module")
def by_function(cases):
    """The two functions forward and backward in ORDER, nothing else in between -> [(width, gMLP results, RCAB results)]."""
    runs = []
    for c in ORDER:
        gm, rc = cases[c]
        runs.append((c, gmlp_by_function(*gm), rcab_by_function(*rc)))
    torch.cuda.synchronize()
    return runs


def test_one_function_serves_both_widths(cases, by_function):
    for c, gm, rc in by_function:
        assert gm[0].shape == GMLP_SHAPE + (c,) and rc[0].shape == RCAB_SHAPE + (c,)
        assert all(bool(torch.isfinite(t).all()) for t in gm + rc), c
    (_, gm_first, rc_first), _, (_, gm_again, rc_again) = by_function
    assert all_bits_equal(gm_again, gm_first) and all_bits_equal(rc_again, rc_first)      # 128 after 256: nothing stale was read
    for c, gm, rc in by_function[:2]:
        assert all_bits_equal(gm, gmlp_direct(*cases[c][0], c)), c
        assert all_bits_equal(rc, rcab_direct(*cases[c][1], c)), c


def test_widths_that_disagree_are_refused_before_a_launch(cases, by_function, monkeypatch):
    launches = []
    launch = ops.launch
    monkeypatch.setattr(ops, "launch", lambda *a, **k: (launches.append(a[0]), launch(*a, **k))[1])
    for c_params, c_act in ((128, 256), (256, 128)):
        (x0, _, _), (y, r, _, _) = cases[c_act]
        (_, gp, _), (_, _, rp, _) = cases[c_params]
        with pytest.raises(BalfHipError, match=rf"x0 must be \[B,Hc,Wc,{c_params}\]"):
            _GmlpTrain.apply(leaf(x0), *[leaf(gp[k]) for k in G.PARAMS])
        with pytest.raises(BalfHipError, match=rf"y must be \[B,Hc,Wc,{c_params}\]"):
            _RcabTrain.apply(leaf(y), leaf(r), *[leaf(rp[k]) for k in R.PARAMS])
        assert not launches
        want = {c: (gm, rc) for c, gm, rc in by_function}[c_act]
        assert all_bits_equal(gmlp_by_function(*cases[c_act][0]), want[0]), (c_params, c_act)
        assert all_bits_equal(rcab_by_function(*cases[c_act][1]), want[1]), (c_params, c_act)
        assert len(launches) == 4                   # each function's forward and backward
        launches.clear()
