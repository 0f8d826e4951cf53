"""Guard-band tests of the entry points that stage 3's training adds, in the pattern of tests/test_train_guard_gpu.py (whose Unit,
Run and checks this file reuses): balf_rcab_train_*_c and balf_gmlp_train_*_c at C = 128 with ``saved`` and the workspace of
exactly the bytes that balf_train_unit_sizes states, and balf_pool_train_* with ``out``, ``which`` and ``dx`` of exactly the bytes
that include/balf_hip.h states, every buffer between two 1 MiB bands of pattern."""
import pytest
import torch

from balf_amd import _lib, ops
from tests import gmlp_train_common as G
from tests import rcab_train_common as R
from tests import stage3_train_common as Sc
from tests.test_train_guard_gpu import DEV, Gmlp, Rcab, _stream, test_exact_size_buffers as check_exact_size_buffers
from tests.test_train_guard_gpu import UNITS
from tests.train_common import NAN_BYTE, Guarded

pytestmark = pytest.mark.gpu
C3 = Sc.C3


class Rcab128(Rcab):
    name = "rcab128"

    def case(self, shape):
        return R.sweep_case(shape, self.seed(shape), device=DEV, c=C3)

    def outputs(self, shape):
        act = tuple(shape) + (C3,)
        out = {"x2": act}
        out.update({"d" + k: ops.rcab_param_shapes(C3)[k] for k in R.PARAMS})
        out["dy"] = act
        return out

    def sizes(self, shape):
        return ops.train_unit_sizes(_lib.UNIT_RCAB, C3, *shape)[::-1]

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_rcab_train_forward_c(p["y"], p["r"], *[p[k] for k in R.PARAMS], *shape, C3, p["x2"], p["saved"],
                                                    p["workspace"], ws_bytes, _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_rcab_train_backward_c(p["dx2"], p["y"], p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], p["saved"],
                                                     *shape, C3, *[p["d" + k] for k in R.PARAMS], p["dy"], p["workspace"], ws_bytes,
                                                     _stream())

    def wrapper(self, case):
        y, r, p, g = case
        f = ops.rcab_train_forward(y, r, [p[k] for k in R.PARAMS], channels=C3)
        b = ops.rcab_train_backward(g, y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], f.saved, want_dy=True, channels=C3)
        out = {"x2": f.x2}
        out.update({k: getattr(b, k) for k in R.GRADS})
        return out


class Gmlp128(Gmlp):
    name = "gmlp128"

    def case(self, shape):
        return G.sweep_case(shape, self.seed(shape), device=DEV, c=C3)

    def outputs(self, shape):
        act = tuple(shape) + (C3,)
        out = {"y": act}
        out.update({"d:" + k: ops.gmlp_param_shapes(C3)[k] for k in G.PARAMS})
        out["dx0"] = act
        return out

    def sizes(self, shape):
        return ops.train_unit_sizes(_lib.UNIT_GMLP, C3, *shape)[::-1]

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_gmlp_train_forward_c(p["x0"], self._array(p, "p:"), *shape, C3, p["y"], p["saved"], p["workspace"],
                                                    ws_bytes, _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_gmlp_train_backward_c(p["dy"], p["x0"], self._array(p, "p:"), p["saved"], *shape, C3,
                                                     self._array(p, "d:"), p["dx0"], p["workspace"], ws_bytes, _stream())

    def wrapper(self, case):
        x0, p, dy = case
        params = [p[k] for k in G.PARAMS]
        f = ops.gmlp_train_forward(x0, params, channels=C3)
        b = ops.gmlp_train_backward(dy, x0, params, f.saved, want_dx0=True, channels=C3)
        out = {"y": f.y, "dx0": b.dx0}
        out.update({"d:" + k: t for k, t in zip(G.PARAMS, b.grads)})
        return out


UNITS_128 = {"rcab128": Rcab128(), "gmlp128": Gmlp128()}


@pytest.mark.parametrize("name,shape", (("rcab128", (3, 3, 5)), ("rcab128", (1, 8, 16)), ("gmlp128", (1, 8, 16))),
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_exact_size_buffers_at_128(name, shape, monkeypatch):
    """Everything test_exact_size_buffers asserts of a unit, of the two units at C = 128: saved and workspace are exactly what
    balf_train_unit_sizes states."""
    monkeypatch.setitem(UNITS, name, UNITS_128[name])
    check_exact_size_buffers(name, shape)


@pytest.mark.parametrize("shape", ((3, 3, 5), (1, 8, 16)), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", (32, C3))
def test_pool_exact_size_buffers(shape, c):
    """``shape`` is the OUTPUT map.  x, g, out, which and dx at exactly their bytes: both return codes 0, every band intact, every
    output the bits of torch's max_pool2d; which is exactly the saved bytes that balf_train_unit_sizes states."""
    b, ho, wo = shape
    x = Sc.pool_cases(shape, c, 11)["random"]
    g = torch.randn((b, ho, wo, c), generator=torch.Generator().manual_seed(12))
    want_out, want_which, want_dx = Sc.pool_reference(x, g)
    ws_bytes, which_bytes = ops.train_unit_sizes(_lib.UNIT_POOL, c, b, 2 * ho, 2 * wo)
    assert (ws_bytes, which_bytes) == (0, b * ho * wo * c)
    buf = {"x": Guarded.of(x.to(DEV)), "g": Guarded.of(g.to(DEV)), "out": Guarded(4 * g.numel(), fill=NAN_BYTE, device=DEV),
           "which": Guarded(which_bytes, fill=NAN_BYTE, device=DEV), "dx": Guarded(4 * x.numel(), fill=NAN_BYTE, device=DEV)}
    l = _lib.lib()
    assert l.balf_pool_train_forward(buf["x"].ptr, b, 2 * ho, 2 * wo, c, buf["out"].ptr, buf["which"].ptr, _stream()) == 0
    assert l.balf_pool_train_backward(buf["g"].ptr, buf["which"].ptr, b, 2 * ho, 2 * wo, c, buf["dx"].ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert not [k for k, v in buf.items() if not v.intact()]
    assert torch.equal(buf["out"].view(torch.int32, want_out.shape).cpu(), want_out.view(torch.int32))
    assert torch.equal(buf["which"].view(torch.uint8, want_which.shape).cpu(), want_which)
    assert torch.equal(buf["dx"].view(torch.int32, want_dx.shape).cpu(), want_dx.view(torch.int32))
