"""All of stage 4 in training form on the GPU: down4.conv.0 and its ReLU (balf_linrelu_train_forward / balf_linrelu_train_backward,
ops.linrelu_train_*, model.stage4_train.TrainableStage4, MLP_MA_DECODER.encode(level="stage3"), utils.train_utils.train_head)
against tests/golden/linrelu_train.npz -- the reference's own modules and autograd, recorded by
tests/golden/make_linrelu_train_golden.py -- and against the float64 restatement of tests/linrelu_train_common.py.  Every output T
is gated by err(T) = max |T - T64| / S_T <= tol_T = max(4 * d_T, 1.1e-6), d_T the reference's own float32 distance from the
restatement (linrelu_train_common.restate64 defines the scales S_T; S_T = 0 demands the exact zero)."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.stage4_train import TrainableStage4, _LinreluTrain
from balf_amd.utils import synth, train_utils
from tests import gmlp_train_common as G
from tests import head_train_common as H
from tests import linrelu_train_common as L
from tests import pair_synth_common as S
from tests import rcab_train_common as R
from tests import train_common as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGIT_TOL = 2e-3                # the gate tests/test_gmlp_train_gpu.py applies to the mixer's logits against the model's forward
# (N, c_in): N = 1, 63, 64, 257 -- partial GEMM tiles in M and a partial last 16-row MFMA tile; N = 960 -- S = 4 slices of which the
# last is short, 15 workgroups of the mask kernel; N = 17408 = 34 x 512 -- two 256-pixel chunks per K slice (rows_per_slice exceeds
# 256 from N = 16385 on), every slice and every block of the mask kernel full
SWEEP = ((1, 128), (63, 128), (960, 128), (17408, 128), (64, 32), (257, 32), (64, 64), (257, 64))
# Where the slice geometry changes (tests/test_train_geometry_host.py asserts each figure).  N = 16899: 512 rows per K slice, S = 34
# with a last slice of 3 rows, a last block of 3 rows.  N = 65536: the last N with blocks of 64 rows, S = 64 and PC = 1024, both caps
# at once.  N = 65537: the first N with blocks of 80 rows -- 1280 rows per slice, S = 52, PC = 820 with a last block of 17 rows -- at
# c_in = 32 and 128, the 16 and the 4 rows in flight of the mask kernel.  Cases and restatement on the device.
LARGE = T.LARGE_SHAPES["linrelu"]
NAN_BYTE = 0xFF                # a buffer of these bytes reads as NaN in float32 and in float64


@pytest.fixture(scope="module")
def fx():
    return L.fixture()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def poison_workspace(n, c_in):
    """Fill the cached workspace of this stream with NaN bytes: a stale word that is read shows in the results."""
    ops._workspace("linrelu_train", DEV, ops.lib().balf_linrelu_train_workspace_bytes(n, c_in)).fill_(NAN_BYTE)


def run(x, w, b, g, want_dx=True, poison=True, y=None):
    """One forward and one backward through ops on the device -> dict of device tensors (GATED).  ``poison``: the workspace and dx
    hold NaN bytes before the calls (the other outputs are fresh ``torch.empty`` tensors of ops).  ``y``: the output handed to the
    backward instead of the forward's own."""
    xd, wd, bd, gd = (t.to(DEV) for t in (x, w, b, g))
    n, c_in = x.numel() // x.shape[-1], x.shape[-1]
    if poison:
        poison_workspace(n, c_in)
    f = ops.linrelu_train_forward(xd, wd, bd)
    dx = want_dx
    if want_dx is True and poison:
        dx = torch.full(xd.shape, float("nan"), device=DEV)
    back = ops.linrelu_train_backward(gd, f.y if y is None else y.to(DEV), xd, wd, want_dx=dx)
    torch.cuda.synchronize()
    return {"y": f.y, "dw": back.dweight, "db": back.dbias, "dx": back.dx}


def check_against(out, res, fx, what, names=L.GATED):
    errs = {k: L.err(out[k], res[k], res["S"][k]) for k in names if out.get(k) is not None}
    print(what, " ".join(f"{k} {e:.2e}" for k, e in errs.items()))                # every figure before any assertion
    bad = {k: (e, float(fx[f"tol_{k}"])) for k, e in errs.items() if not (np.isfinite(e) and e <= float(fx[f"tol_{k}"]))}
    assert not bad, (what, bad)
    return errs


_CASES = {}


def case64(fx, name):
    """A fixture case and its float64 restatement, computed once."""
    if name not in _CASES:
        c = L.fixture_case(fx, name)
        _CASES[name] = (c, L.restate64(*c))
    return _CASES[name]


@pytest.mark.parametrize("name", L.FIXTURE_CASES)
def test_fixture_parity(fx, name):
    (x, w, b, g), res = case64(fx, name)
    out = run(x, w, b, g)
    assert all(out[k] is not None for k in L.GATED)
    check_against(out, res, fx, name)
    assert bool(((out["y"].cpu().reshape(res["h"].shape) > 0) == (res["h"] > 0)).all())       # the mask of the restatement
    if name == "edges":
        y = out["y"].cpu()
        assert bool((y[L.EDGES_ZERO_ROW, :8] == 0).all())       # pre-activations that are exactly 0, with a non-zero g on them
        for c in (L.EDGES_DEAD, 200):                           # dead on every pixel, 1e30 in g: exact zeros
            assert bool((y[:, c] == 0).all()) and float(out["db"][c]) == 0.0 and bool((out["dw"][c] == 0).all())
        assert all(bool(torch.isfinite(out[k]).all()) for k in L.GATED)


_LARGEST = {}


def largest():
    """The last case of LARGE on the device and its first run, made once -> (case, outputs)."""
    if not _LARGEST:
        n, c_in = LARGE[-1]
        c = L.sweep_case(n, c_in, n + c_in, device=DEV)
        _LARGEST.update(case=c, out=run(*c))
    return _LARGEST["case"], _LARGEST["out"]


@pytest.mark.parametrize("n,c_in", SWEEP + LARGE, ids=lambda v: str(v))
def test_shape_sweep(fx, n, c_in):
    what = f"N {n} c_in {c_in}"
    if (n, c_in) not in LARGE:
        x, w, b, g = L.sweep_case(n, c_in, n + c_in)
        res = L.restate64(x, w, b, g)
        out = run(x, w, b, g)
    else:                       # the same gates with the case, the float64 restatement and the float32 composition on the device
        if (n, c_in) == LARGE[-1]:
            (x, w, b, g), out = largest()
        else:
            x, w, b, g = L.sweep_case(n, c_in, n + c_in, device=DEV)
            out = run(x, w, b, g)
        res = L.restate64(x, w, b, g)
        y, grads = L.compose_f32(x, w, b, g)
        T.composition_figures(what, dict(grads, y=y), res, L.GATED, measure=L.err)
    check_against(out, res, fx, what)
    assert bool((out["y"].double().to(res["y"].device) == res["y"]).all())     # every pre-activation of the sweep is exact in float32


def test_largest_shape_gives_the_same_bits_again():
    """The fixed summation order over PC = 820 column blocks of 80 rows and S = 52 slabs."""
    c, a = largest()
    b = run(*c)
    for k in L.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_derivative_at_zero_and_select_under_dead_units():
    """The backward takes the mask from the y it is given: +0, -0 and negative values are dead, and whatever g holds there -- NaN,
    infinities, 1e38 -- never reaches a sum.  The outputs are, bit for bit, those of the same call with zeros in g's dead places."""
    n, c_in = 257, 128
    x, w, b, g = L.sweep_case(n, c_in, 5)
    gen = torch.Generator().manual_seed(9)
    y = torch.rand((n, 2 * c_in), generator=gen) + 0.5
    kind = torch.randint(0, 8, (n, 2 * c_in), generator=gen)
    y[kind == 0] = 0.0
    y[kind == 1] = -0.0
    y[kind == 2] = -1.0
    y[:, 17] = 0.0                                               # a column that is dead on every pixel
    dead = ~(y > 0)
    clean = torch.where(dead, torch.zeros_like(g), g)
    bad = g.clone()
    junk = torch.tensor([float("nan"), float("inf"), float("-inf"), 3e38])
    bad[dead] = junk[torch.randint(0, 4, (int(dead.sum()),), generator=gen)]
    a, c = run(x, w, b, bad, y=y), run(x, w, b, clean, y=y)
    for k in L.GRADS:
        assert bool(torch.isfinite(a[k]).all()) and bits_equal(a[k], c[k]), k
    assert float(a["db"][17]) == 0.0 and bool((a["dw"][17] == 0).all())
    # against the float64 formulas with that mask
    gm = clean.double()
    want = {"db": gm.sum(0), "dw": gm.T @ x.double(), "dx": gm @ w.double()}
    scale = {"db": gm.abs().sum(0).max(), "dw": (gm.abs().T @ x.double().abs()).max(), "dx": (gm.abs() @ w.double().abs()).max()}
    for k in L.GRADS:
        assert L.err(a[k], want[k], float(scale[k])) <= 1.1e-6, k


def test_bitwise_repeatability():
    c = L.sweep_case(960, 128, 50)
    a, b = run(*c), run(*c)
    for k in L.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_independence_of_requests():
    c = L.sweep_case(960, 128, 51)
    full = run(*c)
    lean = run(*c, want_dx=False)
    assert lean["dx"] is None
    for k in ("y", "dw", "db"):
        assert bits_equal(full[k], lean[k]), k
    # dx into a caller's tensor: the same bits, the same object
    mine = torch.full(c[0].shape, float("nan"), device=DEV)
    into = run(*c, want_dx=mine)
    assert into["dx"] is mine and bits_equal(mine, full["dx"])


def test_graph_capture():
    n, c_in = 257, 64
    cases = [L.sweep_case(n, c_in, 60 + i) for i in range(3)]
    static = dict(zip("xwbg", (t.to(DEV) for t in cases[0])))

    def step():
        s = static
        f = ops.linrelu_train_forward(s["x"], s["w"], s["b"])
        back = ops.linrelu_train_backward(s["g"], f.y, s["x"], s["w"], want_dx=True)
        return f.y, back.dweight, back.dbias, back.dx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        outs = step()
    for case in cases[1:]:
        for k, v in zip("xwbg", case):
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run(*case, poison=False)
        for a, k in zip(outs, L.GATED):
            assert bits_equal(a, want[k]), k


def synthetic_model(seed, precision):
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(seed))
    model.precision = precision
    return model.eval().to(DEV)


def conv0_of(model):
    conv0 = model.down4.conv[0]
    return conv0.weight.detach().float().contiguous(), conv0.bias.detach().float().contiguous()


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
def test_forward_on_stage3_is_the_x0_of_the_model(precision):
    """On both kernel families: the stage-3 level is the third stage view, and this layer on it gives the bits of level "gmlp"."""
    model = synthetic_model(3, precision)
    g = torch.Generator().manual_seed(12)
    x = torch.rand((3, 3, 64, 128), generator=g).to(DEV)
    before = model.encode(x)
    x3 = model.encode(x, level="stage3")
    assert model.effective_precision == precision
    assert x3.shape == (3, 8, 16, 128) and x3.dtype == torch.float32 and not x3.requires_grad and x3.is_contiguous()
    model(x)
    assert bits_equal(x3, model.stage_view(3, 64, 128)[2])
    x0 = ops.linrelu_train_forward(x3, *conv0_of(model)).y
    assert bits_equal(x0, model.encode(x, level="gmlp"))
    assert bits_equal(model.encode(x), before)                  # nothing of the forward's state was changed


def test_encode_stage3_in_chunks_is_the_concatenation():
    model = synthetic_model(3, "fp32")
    g = torch.Generator().manual_seed(10)
    x = torch.rand((3, 3, 64, 128), generator=g).to(DEV)
    whole = model.encode(x, level="stage3")
    parts = [model.encode(x[i:i + 1], level="stage3") for i in range(3)]
    halves = model.encode(x, chunk=2, level="stage3")
    assert bits_equal(whole, torch.cat(parts)) and bits_equal(halves, whole)
    with pytest.raises(ValueError, match="'stage3'"):
        model.encode(x, level="x1")


def test_eval_mode():
    """TrainableStage4 in eval() on the stage-3 level gives the model's logits, without a graph and without touching BatchNorm."""
    model = synthetic_model(2, "fp32")
    g = torch.Generator().manual_seed(13)
    x = torch.rand((2, 3, 64, 64), generator=g).to(DEV)
    stage = TrainableStage4.from_model(model)
    stage.eval()
    assert not stage.mixer.training and not stage.mixer.tail.training and not stage.mixer.tail.head.training
    x3 = model.encode(x, level="stage3")
    out = stage(x3.clone().requires_grad_())
    assert out["logits"].grad_fn is None and int(stage.mixer.tail.head.norm.num_batches_tracked) == 0
    want = model(x)["logits"]
    e = float((out["logits"] - want).abs().max())
    print(f"eval logits {e:.2e}")
    assert e <= LOGIT_TOL
    # the same arithmetic as the pieces: the eval mixer on the ops' x0 gives the same bits
    x0 = ops.linrelu_train_forward(x3, *[t.detach() for t in stage.conv0_parameters()]).y
    assert bits_equal(out["logits"], stage.mixer(x0)["logits"])
    assert stage(x3, want_prob=False)["prob"] is None


def test_autograd_path_against_the_reference(fx):
    """Case ``model`` through TrainableStage4 -- conv.0, the layer, the block and the head of synthetic_state_dict(0) -- from the
    dlogits of the reference's loss, as the recorder did, with ONE backward(): autograd adds the three paths into x0 before this
    layer's backward runs, and conv.0's two gradients and x3.grad must be the reference's."""
    (x, w, b, g), res = case64(fx, "model")
    stage = TrainableStage4.from_model(synthetic_model(0, "fp32"))
    assert bits_equal(stage.conv0.weight.detach().cpu(), w)
    xd = x.to(DEV).requires_grad_()
    out = stage(xd)
    assert out["logits"].grad_fn is not None and not out["prob"].requires_grad
    (out["logits"] * torch.from_numpy(fx["model.dlogits"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert int(stage.mixer.tail.head.norm.num_batches_tracked) == 1
    got = {"dw": stage.conv0.weight.grad, "db": stage.conv0.bias.grad, "dx": xd.grad}
    errs = {k: L.err(got[k], torch.from_numpy(fx[f"model.{k}"]), res["S"][k]) for k in L.GRADS}
    print("model", " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e <= float(fx[f"tol_{k}"])}
    assert not bad, bad
    # no gradient wanted for x3: dx is not asked for, the parameter gradients are the same bits
    stage.zero_grad()
    gd = g.to(DEV)
    _LinreluTrain.apply(xd.detach(), *stage.conv0_parameters()).backward(gd)
    lean = [t.grad.clone() for t in stage.conv0_parameters()]
    stage.zero_grad()
    x2 = xd.detach().clone().requires_grad_()
    _LinreluTrain.apply(x2, *stage.conv0_parameters()).backward(gd)
    assert x2.grad is not None and all(bits_equal(a, t.grad) for a, t in zip(lean, stage.conv0_parameters()))


def test_train_stage4_end_to_end():
    """The chunk of tests/test_head_train_gpu.py: one pair of 64 x 64 windows with dense labels, presented six times to
    Adam(lr = 1e-3), here through all of stage 4 and the head."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    chunk = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(chunk) == 1 and chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = synthetic_model(2, "fp32")
    x = chunk[0][0]
    before = train_utils.check_val_anchor_loss(chunk, model, DEV)
    x0_before = model.encode(x, level="gmlp")
    stage = TrainableStage4.from_model(model)
    params = list(stage.parameters())
    assert stage.encode_level == "stage3" and len(params) == 44 and sum(p.numel() for p in params) == 949379
    key = model._weights_key(DEV)
    opt = torch.optim.Adam(stage.parameters(), lr=1e-3)
    gpu = [train_utils.train_head(chunk, model, stage, opt, DEV, noise=False) for _ in range(6)]
    assert model._weights_key(DEV) == key                       # the model was not touched: no re-pack while training
    assert int(stage.mixer.tail.head.norm.num_batches_tracked) == 12
    # the same six presentations in float64 on the CPU, from the same features
    feats = [(model.encode(b[0], level="stage3").cpu(), model.encode(b[1], level="stage3").cpu(), b[2].cpu(), b[3].cpu()) for b in chunk]
    sd = synth.synthetic_state_dict(2)
    hp, running = H.params_of(sd)
    cpu = L.train64(feats, L.params_of(sd), G.params_of(sd), R.params_of(sd), hp, running, 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; GPU", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    print("largest difference", max(abs(a - b) for a, b in zip(gpu, cpu)))
    # the fourth decimal, the tolerance of test_train_mixer_tail_end_to_end: Adam's update is a continuous function of the
    # gradients, which agree to ~1e-6 of their scales, and the float32 loss itself carries ~1e-7 of a value of a few units
    assert max(abs(a - b) for a, b in zip(gpu, cpu)) <= 5e-5
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    assert float((stage.conv0.weight.detach().cpu() - sd[L.SD_PREFIX + "weight"]).abs().max()) > 1e-4     # conv.0 itself moved
    stage.commit(model)
    assert model._weights_key(DEV) != key
    # level "gmlp" takes conv.0 from the model: it shows the new weights, and is this layer on the unchanged stage-3 output
    x0_after = model.encode(x, level="gmlp")
    assert not bits_equal(x0_after, x0_before)
    assert bits_equal(x0_after, ops.linrelu_train_forward(model.encode(x, level="stage3"), *conv0_of(model)).y)
    assert bits_equal(conv0_of(model)[0], stage.conv0.weight.detach())
    got, want = model.eval()(x)["logits"], stage.eval()(model.encode(x, level="stage3"))["logits"]
    assert float((got - want).abs().max()) <= LOGIT_TOL
    after = train_utils.check_val_anchor_loss(chunk, model, DEV)
    print(f"check_val_anchor_loss before {before:.4f} after {after:.4f}")
    assert after < before


def test_argument_errors():
    """Each is a return code of the library; nothing is launched (the outputs keep their NaN)."""
    l = ops.lib()
    n, c_in = 63, 128
    x, w, b, g = (t.to(DEV) for t in L.sweep_case(n, c_in, 70))
    y = torch.full((n, 2 * c_in), float("nan"), device=DEV)
    dw, db, dx = (torch.full(s, float("nan"), device=DEV) for s in ((2 * c_in, c_in), (2 * c_in,), (n, c_in)))
    ws = torch.empty(l.balf_linrelu_train_workspace_bytes(n, c_in), dtype=torch.uint8, device=DEV)
    ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3
    p = lambda t: t.data_ptr()                                   # noqa: E731

    def fwd(dims=(n, c_in), xx=p(x), ww=p(w), bb=p(b), out=p(y)):
        return l.balf_linrelu_train_forward(xx, ww, bb, *dims, out, None)

    def bwd(dims=(n, c_in), gg=p(g), yy=p(y), xx=p(x), ww=p(w), o_dw=p(dw), o_db=p(db), o_dx=p(dx), work=p(ws), wb=ws.numel()):
        return l.balf_linrelu_train_backward(gg, yy, xx, ww, *dims, o_dw, o_db, o_dx, work, wb, None)

    assert l.balf_error_string(ERR_SHAPE) and l.balf_error_string(ERR_WORKSPACE)
    for bad in (0, 16, 96, 256):
        assert fwd(dims=(n, bad)) == ERR_ARG and bwd(dims=(n, bad)) == ERR_ARG and l.balf_linrelu_train_workspace_bytes(n, bad) == 0
    for bad in (0, -1, (1 << 24) + 1):
        assert fwd(dims=(bad, c_in)) == ERR_SHAPE and bwd(dims=(bad, c_in)) == ERR_SHAPE
        assert l.balf_linrelu_train_workspace_bytes(bad, c_in) == 0
    assert fwd(xx=None) == ERR_ARG and fwd(ww=None) == ERR_ARG and fwd(bb=None) == ERR_ARG and fwd(out=None) == ERR_ARG
    assert bwd(gg=None) == ERR_ARG and bwd(yy=None) == ERR_ARG and bwd(xx=None) == ERR_ARG and bwd(ww=None) == ERR_ARG
    assert bwd(o_dw=None) == ERR_ARG and bwd(o_db=None) == ERR_ARG and bwd(work=None) == ERR_ARG
    assert fwd(xx=p(x) + 4) == ERR_ARG and fwd(out=p(y) + 8) == ERR_ARG and fwd(ww=p(w) + 4) == ERR_ARG
    assert bwd(gg=p(g) + 4) == ERR_ARG and bwd(o_dx=p(dx) + 4) == ERR_ARG and bwd(work=p(ws) + 8) == ERR_ARG and bwd(o_db=p(db) + 4) == ERR_ARG
    assert bwd(wb=ws.numel() - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, dw, db, dx))
    assert fwd() == 0 and bwd() == 0                            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (y, dw, db, dx))
    assert bwd(o_dx=None) == 0
    # the wrappers refuse from the metadata
    with pytest.raises(ops.BalfHipError):
        ops.linrelu_train_forward(torch.zeros((4, 96), device=DEV), w, b)
