"""Guard-band tests of the training path's C ABI: where the kernels write.

The parity tests of the four training units go through balf_amd/ops.py, which hands the library a cached workspace that is
almost always larger than ``*_workspace_bytes`` and fresh ``torch.empty`` outputs that the caching allocator pads and packs next
to other live blocks: a store a few rows past N, a slab one element longer than make_layout reserved or a size query that
under-reports lands in slack, and every tolerance still passes.  Here every caller-owned buffer -- inputs, parameters, gradients,
outputs, ``saved``, workspace -- is a train_common.Guarded of EXACTLY its documented size (include/balf_hip.h) between two 1 MiB
bands of pattern, the calls go straight through ctypes, and after a forward and a backward

  * both return codes are 0 and every band of every buffer is intact;
  * every output has the bits that the ops wrapper returns for the same inputs (the header promises results that depend on the
    shape alone): every element was written, and nothing depends on slack or on what a buffer held before -- outputs, ``saved``
    and the workspace start as 0xFF bytes, NaN in float32 and float64;
  * a second forward and backward into the same ``saved`` and workspace, not poisoned again, give the same bits;
  * one byte less of workspace is refused with BALF_ERR_WORKSPACE and nothing is written;
  * with the optional outputs NULL the others keep their bits, and all bands stay intact.

The inputs are each unit's sweep_case at the seeds of its test_shape_sweep, which gates the same inputs against the float64
restatement; the shapes are train_common.GUARD_SHAPES.  The stage-view family (balf_forward_stage_view, balf_forward_rcab_inputs,
balf_forward_gmlp_input) gets the same treatment after a resident forward, and the paths that look at a pointer's alignment run
with buffers that start 4 bytes behind a 16-byte boundary."""
import ctypes as C

import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.model import get_model
from balf_amd.utils import synth
from tests import gmlp_train_common as G
from tests import head_train_common as H
from tests import linrelu_train_common as L
from tests import rcab_train_common as R
from tests import train_common as T
from tests.train_common import NAN_BYTE, Guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ERR_WORKSPACE = -3                          # BALF_ERR_WORKSPACE


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


class Unit:
    """One training unit behind the C ABI.  A subclass names its buffers:

    ``inputs(case)``      name -> float32 device tensor that the calls only read (the running statistics of the head, which its
                          forward updates in place, are in ``inout``);
    ``outputs(shape)``    name -> shape of every float32 output, the forward's first;
    ``optional``          the outputs that may be NULL;
    ``sizes(shape)``      (saved bytes or None, workspace bytes);
    ``forward`` / ``backward``: one call on a dict name -> pointer (None: NULL) -> return code;
    ``wrapper(case)``     the same outputs through balf_amd.ops."""
    name = ""
    optional = ()
    inout = ()
    forward_takes_workspace = True

    def pixels(self, shape):
        return T.guard_shape_pixels(self.name, shape)

    def seed(self, shape):
        return 7 + shape[1] * 100 + shape[2]                    # the seeds of the units' test_shape_sweep


class Run:
    """The guarded buffers of one (unit, shape, case) and the calls on them."""

    def __init__(self, unit, shape, case, offsets=None):
        offsets = offsets or {}
        self.unit, self.shape = unit, shape
        self.initial = unit.inputs(case)
        self.out_shapes = unit.outputs(shape)
        assert set(offsets) <= set(self.initial) | set(self.out_shapes), offsets
        self.buf = {k: Guarded.of(t, offset=offsets.get(k, 0)) for k, t in self.initial.items()}
        for k, s in self.out_shapes.items():
            if k not in unit.inout:
                self.buf[k] = Guarded(4 * _numel(s), fill=NAN_BYTE, offset=offsets.get(k, 0), device=DEV)
        saved_bytes, self.ws_bytes = unit.sizes(shape)
        assert self.ws_bytes > 0 and saved_bytes != 0, (unit.name, shape)
        if saved_bytes is not None:
            self.buf["saved"] = Guarded(saved_bytes, fill=NAN_BYTE, device=DEV)
        self.buf["workspace"] = Guarded(self.ws_bytes, fill=NAN_BYTE, device=DEV)
        self.outs = tuple(self.out_shapes)

    def what(self):
        return f"{self.unit.name} {self.shape}"

    def reset_outputs(self):
        """Outputs back to 0xFF bytes, the in-out tensors back to their initial values."""
        for k in self.outs:
            if k in self.unit.inout:
                self.buf[k].load(self.initial[k])
            else:
                self.buf[k].fill(NAN_BYTE)

    def pointers(self, omit=()):
        return {k: (None if k in omit else g.ptr) for k, g in self.buf.items()}

    def step(self, omit=(), poison_workspace=True):
        """Forward, then backward (the workspace poisoned again in between) -> the two return codes, synchronised."""
        p = self.pointers(omit)
        rc_f = self.unit.forward(p, self.shape, self.ws_bytes)
        if poison_workspace:
            self.buf["workspace"].fill(NAN_BYTE)
        rc_b = self.unit.backward(p, self.shape, self.ws_bytes)
        torch.cuda.synchronize()
        return rc_f, rc_b

    def trampled(self):
        """The names of the buffers with a band that does not hold its pattern any more."""
        return [k for k, g in self.buf.items() if not g.intact()]

    def bits(self, omit=()):
        return {k: self.buf[k].view(torch.int32, self.out_shapes[k]).clone() for k in self.outs if k not in omit}

    def unwritten(self, names):
        """Of ``names``, the outputs that do not hold what reset_outputs left there."""
        bad = []
        for k in names:
            if k in self.unit.inout:
                ok = _same_bits(self.buf[k].view(torch.float32, self.out_shapes[k]), self.initial[k])
            else:
                ok = self.buf[k].holds(NAN_BYTE)
            if not ok:
                bad.append(k)
        return bad


def differing(got, want):
    return [k for k in got if not bool((got[k] == want[k].view(torch.int32).reshape(got[k].shape)).all())]


# ---- the four units ---------------------------------------------------------------------------------------------------------------
class Head(Unit):
    name = "head"
    optional = ("prob", "running_mean", "running_var", "dx2")
    inout = ("running_mean", "running_var")
    forward_outs = ("logits", "prob", "running_mean", "running_var")

    def case(self, shape):
        return H.sweep_case(shape, self.seed(shape), device=DEV)

    def inputs(self, case):
        x2, p, dlogits, running = case
        return dict(p, x2=x2, dlogits=dlogits, running_mean=running[0], running_var=running[1])

    def outputs(self, shape):
        b, hc, wc = shape
        return {"logits": (b, 65, hc, wc), "prob": (b, 8 * hc, 8 * wc), "running_mean": (65,), "running_var": (65,),
                "dw2": (256, 256), "db2": (256,), "dwd": (65, 256), "dbd": (65,), "dgamma": (65,), "dbeta": (65,),
                "dx2": (b, hc, wc, 256)}

    def sizes(self, shape):
        n = self.pixels(shape)
        return _lib.lib().balf_head_train_saved_bytes(n), _lib.lib().balf_head_train_workspace_bytes(n)

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_head_train_forward(p["x2"], p["w2"], p["b2"], p["wd"], p["bd"], p["gamma"], p["beta"], *shape, H.EPS, 0,
                                                  None, p["logits"], p["prob"], p["running_mean"], p["running_var"], H.MOMENTUM,
                                                  p["saved"], p["workspace"], ws_bytes, _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_head_train_backward(p["dlogits"], p["x2"], p["w2"], p["wd"], p["gamma"], p["saved"], *shape, p["dw2"],
                                                   p["db2"], p["dwd"], p["dbd"], p["dgamma"], p["dbeta"], p["dx2"], p["workspace"],
                                                   ws_bytes, _stream())

    def wrapper(self, case):
        x2, p, dlogits, running = case
        rm, rv = running[0].clone(), running[1].clone()
        f = ops.head_train_forward(x2, p["w2"], p["b2"], p["wd"], p["bd"], p["gamma"], p["beta"], eps=H.EPS, want_prob=True,
                                   running_mean=rm, running_var=rv, momentum=H.MOMENTUM)
        b = ops.head_train_backward(dlogits, x2, p["w2"], p["wd"], p["gamma"], f.saved, want_dx2=True)
        out = {"logits": f.logits, "prob": f.prob, "running_mean": rm, "running_var": rv}
        out.update({k: getattr(b, k) for k in H.GRADS})
        return out


class Rcab(Unit):
    name = "rcab"
    optional = ("dy",)
    forward_outs = ("x2",)

    def case(self, shape):
        return R.sweep_case(shape, self.seed(shape), device=DEV)

    def inputs(self, case):
        y, r, p, g = case
        return dict(p, y=y, r=r, dx2=g)

    def outputs(self, shape):
        act = tuple(shape) + (256,)
        out = {"x2": act}
        out.update({"d" + k: ops._RCAB_PARAM_SHAPES[k] for k in R.PARAMS})
        out["dy"] = act
        return out

    def sizes(self, shape):
        return _lib.lib().balf_rcab_train_saved_bytes(*shape), _lib.lib().balf_rcab_train_workspace_bytes(*shape)

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_rcab_train_forward(p["y"], p["r"], *[p[k] for k in R.PARAMS], *shape, p["x2"], p["saved"], p["workspace"],
                                                  ws_bytes, _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_rcab_train_backward(p["dx2"], p["y"], p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], p["saved"],
                                                   *shape, *[p["d" + k] for k in R.PARAMS], p["dy"], p["workspace"], ws_bytes,
                                                   _stream())

    def wrapper(self, case):
        y, r, p, g = case
        f = ops.rcab_train_forward(y, r, [p[k] for k in R.PARAMS])
        b = ops.rcab_train_backward(g, y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], f.saved, want_dy=True)
        out = {"x2": f.x2}
        out.update({k: getattr(b, k) for k in R.GRADS})
        return out


class Gmlp(Unit):
    name = "gmlp"
    optional = ("dx0",)
    forward_outs = ("y",)

    def case(self, shape):
        return G.sweep_case(shape, self.seed(shape), device=DEV)

    def inputs(self, case):
        x0, p, dy = case
        return dict({"p:" + k: p[k] for k in G.PARAMS}, x0=x0, dy=dy)

    def outputs(self, shape):
        act = tuple(shape) + (256,)
        out = {"y": act}
        out.update({"d:" + k: ops._GMLP_PARAM_SHAPES[k] for k in G.PARAMS})
        out["dx0"] = act
        return out

    def sizes(self, shape):
        return _lib.lib().balf_gmlp_train_saved_bytes(*shape), _lib.lib().balf_gmlp_train_workspace_bytes(*shape)

    @staticmethod
    def _array(p, prefix):
        return (C.c_void_p * len(G.PARAMS))(*[p[prefix + k] for k in G.PARAMS])

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_gmlp_train_forward(p["x0"], self._array(p, "p:"), *shape, p["y"], p["saved"], p["workspace"], ws_bytes,
                                                  _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_gmlp_train_backward(p["dy"], p["x0"], self._array(p, "p:"), p["saved"], *shape, self._array(p, "d:"),
                                                   p["dx0"], p["workspace"], ws_bytes, _stream())

    def wrapper(self, case):
        x0, p, dy = case
        params = [p[k] for k in G.PARAMS]
        f = ops.gmlp_train_forward(x0, params)
        b = ops.gmlp_train_backward(dy, x0, params, f.saved, want_dx0=True)
        out = {"y": f.y, "dx0": b.dx0}
        out.update({"d:" + k: t for k, t in zip(G.PARAMS, b.grads)})
        return out


class Linrelu(Unit):
    name = "linrelu"
    optional = ("dx",)
    forward_outs = ("y",)
    forward_takes_workspace = False

    def seed(self, shape):
        return shape[0] + shape[1]

    def case(self, shape):
        return L.sweep_case(*shape, self.seed(shape), device=DEV)

    def inputs(self, case):
        x, w, b, g = case
        return {"x": x, "w": w, "b": b, "g": g}

    def outputs(self, shape):
        n, c = shape
        return {"y": (n, 2 * c), "dw": (2 * c, c), "db": (2 * c,), "dx": (n, c)}

    def sizes(self, shape):
        return None, _lib.lib().balf_linrelu_train_workspace_bytes(*shape)

    def forward(self, p, shape, ws_bytes):
        return _lib.lib().balf_linrelu_train_forward(p["x"], p["w"], p["b"], *shape, p["y"], _stream())

    def backward(self, p, shape, ws_bytes):
        return _lib.lib().balf_linrelu_train_backward(p["g"], p["y"], p["x"], p["w"], *shape, p["dw"], p["db"], p["dx"], p["workspace"],
                                                      ws_bytes, _stream())

    def wrapper(self, case):
        x, w, b, g = case
        y = ops.linrelu_train_forward(x, w, b).y
        back = ops.linrelu_train_backward(g, y, x, w, want_dx=True)
        return {"y": y, "dw": back.dweight, "db": back.dbias, "dx": back.dx}


UNITS = {u.name: u for u in (Head(), Rcab(), Gmlp(), Linrelu())}
CASES = [(name, shape) for name in UNITS for shape, _ in T.GUARD_SHAPES[name]]


@pytest.mark.parametrize("name,shape", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_exact_size_buffers(name, shape):
    unit = UNITS[name]
    case = unit.case(shape)
    want = unit.wrapper(case)
    torch.cuda.synchronize()
    run = Run(unit, shape, case)
    what = run.what()

    # every buffer at exactly its documented size, outputs, saved and workspace poisoned
    assert run.step() == (0, 0), what
    assert not run.trampled(), f"{what}: written outside {run.trampled()}"
    first = run.bits()
    assert not differing(first, want), f"{what}: not the bits of the ops wrapper: {differing(first, want)}"

    # the reuse of a training loop: the same saved and workspace again, as the first step left them
    run.reset_outputs()
    assert run.step(poison_workspace=False) == (0, 0), what
    assert not run.trampled(), f"{what}, second step: written outside {run.trampled()}"
    assert not differing(run.bits(), first), f"{what}, second step: other bits in {differing(run.bits(), first)}"

    # one byte less of workspace is refused, and nothing is written
    run.reset_outputs()
    p = run.pointers()
    checked = run.outs
    if unit.forward_takes_workspace:
        assert unit.forward(p, shape, run.ws_bytes - 1) == ERR_WORKSPACE, what
    else:
        checked = tuple(k for k in run.outs if k not in unit.forward_outs)
    assert unit.backward(p, shape, run.ws_bytes - 1) == ERR_WORKSPACE, what
    torch.cuda.synchronize()
    assert not run.unwritten(checked), f"{what}: a refused call wrote {run.unwritten(checked)}"

    # the optional outputs NULL: the others keep their bits, the buffers that were not passed keep their fill
    run.reset_outputs()
    assert run.step(omit=unit.optional) == (0, 0), what
    assert not run.trampled(), f"{what}, optional outputs NULL: written outside {run.trampled()}"
    lean = run.bits(omit=unit.optional)
    assert not differing(lean, first), f"{what}, optional outputs NULL: other bits in {differing(lean, first)}"
    assert not run.unwritten(unit.optional), f"{what}: a NULL output was written: {run.unwritten(unit.optional)}"


# ---- the paths that look at a pointer's alignment --------------------------------------------------------------------------------
def _aligned_and_offset(unit, shape, offset_sets):
    """The all-aligned run and one run per set of buffers that start 4 bytes behind a 16-byte boundary -> the failures."""
    case = unit.case(shape)
    base = Run(unit, shape, case)
    assert base.step() == (0, 0) and not base.trampled(), base.what()
    want = base.bits()
    del base
    bad = []
    for names in offset_sets:
        run = Run(unit, shape, case, offsets={k: 4 for k in names})
        assert all(run.buf[k].ptr % 16 == 4 for k in names)
        rcs = run.step()
        if rcs != (0, 0):
            bad.append((names, "return codes", rcs))
        if run.trampled():
            bad.append((names, "written outside", run.trampled()))
        if differing(run.bits(), want):
            bad.append((names, "other bits in", differing(run.bits(), want)))
    return bad


@pytest.mark.parametrize("shape", ((2, 7, 9), (1, 129, 131)), ids=lambda s: "x".join(map(str, s)))
def test_rcab_backward_with_unaligned_dx2_and_dy(shape):
    """ln_bwd_kernel takes dx2 with 16-byte or 4-byte loads (vec_g) and stores dy with 16-byte or 4-byte stores (vec_dy), each by
    its own pointer: the three combinations with an unaligned pointer give the bits of the aligned run, inside the buffers."""
    bad = _aligned_and_offset(UNITS["rcab"], shape, (("dx2",), ("dy",), ("dx2", "dy")))
    assert not bad, (shape, bad)


def test_head_forward_with_unaligned_prob():
    """normalize_kernel stores prob as float4 pairs or as single floats, by the pointer's alignment."""
    bad = _aligned_and_offset(UNITS["head"], (1, 5, 13), (("prob",),))
    assert not bad, bad


# ---- the stage-view family -------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(precision):
    if precision not in _MODELS:
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(synth.synthetic_state_dict(3))
        m.precision = precision
        _MODELS[precision] = m.eval().to(DEV)
    return _MODELS[precision]


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
@pytest.mark.parametrize("b,hp,wp", ((2, 64, 128), (1, 64, 448)), ids=("2x64x128", "1x64x448"))
def test_stage_views_stay_inside_their_buffers(precision, b, hp, wp):
    l = _lib.lib()
    model = _model(precision)
    x = torch.rand((b, 3, hp, wp), generator=torch.Generator().manual_seed(11 + wp)).to(DEV)
    # what the module and the ops wrappers give, on the cached workspace
    model(x)
    model.fp16_guard_check()
    assert model.effective_precision == precision               # the path under test is the one that ran
    prec = model._code_of(precision)
    nbytes = l.balf_forward_workspace_bytes(b, hp, wp)
    conv0 = model.down4.conv[0]
    w0, b0 = conv0.weight.detach().float().contiguous(), conv0.bias.detach().float().contiguous()
    act = (b, hp // 8, wp // 8, 256)
    want = {f"stage{i + 1}": t for i, t in enumerate(model.stage_view(b, hp, wp))}
    cached = ops._workspace("forward", DEV, nbytes)
    want.update({k: torch.empty(act, device=DEV) for k in ("y", "r", "x0")})
    ops.rcab_inputs(prec, cached, b, hp, wp, w0, b0, want["y"], want["r"])
    ops.gmlp_input(prec, cached, b, hp, wp, w0, b0, want["x0"])
    torch.cuda.synchronize()

    # the same forward into a workspace of exactly balf_forward_workspace_bytes, then the three calls into exact-size buffers
    blob = model.packed_weights(DEV, precision)
    ws, xin = Guarded(nbytes, fill=NAN_BYTE, device=DEV), Guarded.of(x)
    prob, logits = Guarded(b * hp * wp * 4, fill=NAN_BYTE, device=DEV), Guarded(b * 65 * (hp // 8) * (wp // 8) * 4, fill=NAN_BYTE, device=DEV)
    assert l.balf_forward(blob.data_ptr(), prec, xin.ptr, b, hp, wp, logits.ptr, prob.ptr, ws.ptr, ws.n, _stream()) == 0
    torch.cuda.synchronize()
    before = ws.bytes().clone()
    buf = {"workspace": ws, "conv0_w": Guarded.of(w0), "conv0_b": Guarded.of(b0)}
    shapes = {}
    for stage in range(1, 5):
        n = l.balf_forward_stage_view_numel(b, hp, wp, stage)
        assert n == want[f"stage{stage}"].numel()
        shapes[f"stage{stage}"] = tuple(want[f"stage{stage}"].shape)
        buf[f"stage{stage}"] = Guarded(4 * n, fill=NAN_BYTE, device=DEV)
        assert l.balf_forward_stage_view(prec, ws.ptr, ws.n, b, hp, wp, stage, buf[f"stage{stage}"].ptr, _stream()) == 0
    for k in ("y", "r", "x0"):
        shapes[k] = act
        buf[k] = Guarded(4 * _numel(act), fill=NAN_BYTE, device=DEV)
    assert l.balf_forward_rcab_inputs(prec, ws.ptr, ws.n, b, hp, wp, buf["conv0_w"].ptr, buf["conv0_b"].ptr, buf["y"].ptr,
                                      buf["r"].ptr, _stream()) == 0
    scratch = None
    if precision == "fp16":                                     # the de-fragmented stage-3 view: B * Hp/8 * Wp/8 * 128 floats
        buf["scratch"] = Guarded(4 * _numel(act) // 2, fill=NAN_BYTE, device=DEV)
        scratch = buf["scratch"].ptr
    assert l.balf_forward_gmlp_input(prec, ws.ptr, ws.n, b, hp, wp, buf["conv0_w"].ptr, buf["conv0_b"].ptr, buf["x0"].ptr, scratch,
                                     _stream()) == 0
    torch.cuda.synchronize()
    what = f"{precision} {(b, hp, wp)}"
    trampled = [k for k, g in buf.items() if not g.intact()]
    assert not trampled, f"{what}: written outside {trampled}"
    got = {k: buf[k].view(torch.int32, s) for k, s in shapes.items()}
    assert not differing(got, want), f"{what}: not the bits of the module's views: {differing(got, want)}"
    assert bool((ws.bytes() == before).all()), f"{what}: the forward's workspace was changed"
    # one byte less than the forward's workspace is refused
    assert l.balf_forward_gmlp_input(prec, ws.ptr, ws.n - 1, b, hp, wp, buf["conv0_w"].ptr, buf["conv0_b"].ptr, buf["x0"].ptr, scratch,
                                     _stream()) == ERR_WORKSPACE
