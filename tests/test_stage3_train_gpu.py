"""Stage 3 in training form on the GPU: the channel-attention block and the multi-axis gated-MLP layer at C = 128
(balf_rcab_train_*_c, balf_gmlp_train_*_c, ops.*(channels=128)), the 2 x 2 max-pool (balf_pool_train_*, ops.pool_train_*),
model.stage3_train.TrainableStage3, MLP_MA_DECODER.encode(level="stage2") and utils.train_utils.train_head with it, against
tests/golden/stage3_train.npz -- the reference's own modules and autograd, recorded by tests/golden/make_stage3_train_golden.py
-- and the float64 restatements of the units (tests/rcab_train_common.py, tests/gmlp_train_common.py at c = 128) and of the
stage (tests/stage3_train_common.py).  Every output T of the two units and of the whole stage is
gated by err(T) = max |T - T64| / S_T <= tol_T = max(4 * d_T, 1.1e-6), d_T the reference's own float32 distance from the
restatement; the pool is exact: the bits of torch's CPU max_pool2d and of its autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.stage3_train import TrainableStage3
from balf_amd.utils import synth, train_utils
from tests import gmlp_train_common as G
from tests import pair_synth_common as S
from tests import rcab_train_common as R
from tests import stage3_train_common as Sc
from tests import train_common as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGIT_TOL = 2e-3                # the gate the sibling tests apply to a module's logits against the model's forward
C3 = Sc.C3
# (B, Hc, Wc).  RCAB: the minimum of two pixels either way, an odd N (a wave of the LayerNorm with one pixel), 63 images of 5
# pixels (a column block over many images), and (1,129,131), N = 16899: 512 rows per K slice, S = 34, PC = 265 column blocks,
# PI = 265 row blocks of the one image.  (2,257,257), N = 132098: the upper regime (2304 rows per slice, blocks of 144 rows, 65 rows
# per image block, image 1 beginning inside a tile); case and restatement on the device.
RCAB_SWEEP = ((1, 1, 2), (2, 1, 1), (3, 3, 5), (63, 1, 5), (1, 129, 131), (2, 257, 257))
GMLP_SWEEP = ((1, 8, 8), (2, 8, 16), (2, 16, 8), (3, 16, 24), (1, 24, 40))
NAN_BYTE = T.NAN_BYTE


@pytest.fixture(scope="module")
def fx():
    return Sc.fixture()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def poison(unit, tag, shape, c=C3):
    """Fill the cached workspace of this stream with NaN bytes: a stale word that is read shows in the results."""
    ops._workspace(tag, DEV, ops.train_unit_sizes(unit, c, *shape)[0]).fill_(NAN_BYTE)


def run_rcab(y, r, p, g, want_dy=True, c=C3):
    yd, rd, gd = (t.to(DEV) for t in (y, r, g))
    pd = {k: v.to(DEV) for k, v in p.items()}
    shape = tuple(y.shape[:3])
    poison(_lib.UNIT_RCAB, "rcab_train", shape, c)
    saved = torch.full((ops.train_unit_sizes(_lib.UNIT_RCAB, c, *shape)[1],), NAN_BYTE, dtype=torch.uint8, device=DEV)
    f = ops.rcab_train_forward(yd, rd, [pd[k] for k in R.PARAMS], saved=saved, channels=c)
    poison(_lib.UNIT_RCAB, "rcab_train", shape, c)
    dy = torch.full(yd.shape, float("nan"), device=DEV) if want_dy else False
    back = ops.rcab_train_backward(gd, yd, pd["ln_g"], pd["wc1"], pd["wc2"], pd["ws0"], pd["ws2"], f.saved, want_dy=dy, channels=c)
    torch.cuda.synchronize()
    return dict(zip(R.GATED, (f.x2,) + tuple(back)))


def run_gmlp(x0, p, g, want_dx0=True, c=C3):
    xd, gd = x0.to(DEV), g.to(DEV)
    params = [p[k].to(DEV) for k in G.PARAMS]
    shape = tuple(x0.shape[:3])
    poison(_lib.UNIT_GMLP, "gmlp_train", shape, c)
    saved = torch.full((ops.train_unit_sizes(_lib.UNIT_GMLP, c, *shape)[1],), NAN_BYTE, dtype=torch.uint8, device=DEV)
    f = ops.gmlp_train_forward(xd, params, saved=saved, channels=c)
    poison(_lib.UNIT_GMLP, "gmlp_train", shape, c)
    dx0 = torch.full(xd.shape, float("nan"), device=DEV) if want_dx0 else False
    back = ops.gmlp_train_backward(gd, xd, params, f.saved, want_dx0=dx0, channels=c)
    torch.cuda.synchronize()
    return dict(zip(G.GATED, (f.y,) + tuple(back.grads) + (back.dx0,)))


def check_against(out, res, fx, unit, what, names):
    errs = {k: Sc.err(out[k], res[k], res["S"][k]) for k in names if out.get(k) is not None}
    print(what, " ".join(f"{k} {e:.2e}" for k, e in errs.items()))                # every figure before any assertion
    bad = {k: (e, Sc.tol(fx, unit, k)) for k, e in errs.items() if not (np.isfinite(e) and e <= Sc.tol(fx, unit, k))}
    assert not bad, (what, bad)
    return max(errs.values())


# ---- the channel-attention block at C = 128 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Sc.RCAB_CASES)
def test_rcab_fixture_cases(fx, name):
    y, r, p, g = Sc.rcab_case(name)
    assert T.inputs_digest(y, r, p, g) == str(fx[f"rcab.{name}.inputs_sha256"])
    out = run_rcab(y, r, p, g)
    check_against(out, R.restate64(y, r, p, g), fx, "rcab", f"rcab128 {name}", R.GATED)
    lean = run_rcab(y, r, p, g, want_dy=False)
    assert lean["dy"] is None and all(bits_equal(out[k], lean[k]) for k in R.GATED[:-1])     # dy not requested: the same bits
    if name == "edges":
        assert bool(torch.isfinite(out["dln_g"][R.EDGES_LN_G0]))                             # finite where ln_g = 0
        assert float(out["dbs0"][R.EDGES_E0]) == 0.0 and bool((out["dws0"][R.EDGES_E0] == 0).all())   # the dead squeeze-excite unit


@pytest.mark.parametrize("shape", RCAB_SWEEP)
def test_rcab_sweep(fx, shape):
    big = shape[0] * shape[1] * shape[2] > 4096
    y, r, p, g = R.sweep_case(shape, 100 + sum(shape), device=DEV if big else None, c=C3)
    out = run_rcab(y, r, p, g)
    check_against(out, R.restate64(y, r, p, g), fx, "rcab", f"rcab128 {shape}", R.GATED)
    again = run_rcab(y, r, p, g, want_dy=False)
    assert all(bits_equal(out[k], again[k]) for k in R.GATED[:-1])


# ---- the gated-MLP layer at C = 128 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Sc.GMLP_CASES)
def test_gmlp_fixture_cases(fx, name):
    x0, p, g = Sc.gmlp_case(name)
    assert T.inputs_digest(x0, p, g) == str(fx[f"gmlp.{name}.inputs_sha256"])
    out = run_gmlp(x0, p, g)
    res = G.restate64(x0, p, g)
    check_against(out, res, fx, "gmlp", f"gmlp128 {name}", G.GATED)
    lean = run_gmlp(x0, p, g, want_dx0=False)
    assert lean["dx0"] is None and all(bits_equal(out[k], lean[k]) for k in G.GATED[:-1])    # dx0 not requested: the same bits
    if name == "layout":
        # the grid map, the block map and the orientation of Wt each change the result: a swap is far outside the gate
        (gl, gu), (bl, bu) = G.BRANCHES
        swapped = dict(p)
        swapped[f"{gl}.{gu}.dense.weight"] = p[f"{gl}.{gu}.dense.weight"].T.contiguous()
        assert Sc.err(G.restate64(x0, swapped)["y"], res["y"], res["S"]["y"]) > 1e-3
        for k in ("dense.weight", "dense.bias"):
            swapped = dict(p)
            swapped[f"{gl}.{gu}.{k}"], swapped[f"{bl}.{bu}.{k}"] = p[f"{bl}.{bu}.{k}"], p[f"{gl}.{gu}.{k}"]
            assert Sc.err(G.restate64(x0, swapped)["y"], res["y"], res["S"]["y"]) > 1e-3


@pytest.mark.parametrize("shape", GMLP_SWEEP)
def test_gmlp_sweep(fx, shape):
    x0, p, g = G.sweep_case(shape, 200 + sum(shape), c=C3)
    out = run_gmlp(x0, p, g)
    check_against(out, G.restate64(x0, p, g), fx, "gmlp", f"gmlp128 {shape}", G.GATED)
    again = run_gmlp(x0, p, g, want_dx0=False)
    assert all(bits_equal(out[k], again[k]) for k in G.GATED[:-1])


# ---- C = 256 through the new entry points --------------------------------------------------------------------------------------
def test_c256_through_the_c_entry_points_is_the_existing_code():
    """One case each: balf_*_train_*_c(C = 256) gives the bits of balf_*_train_* (which call it), through buffers of the sizes of
    the existing queries, which balf_train_unit_sizes repeats."""
    l = ops.lib()
    shape = (2, 8, 16)
    y, r, p, g = (T.to_device(t, DEV) for t in R.sweep_case(shape, 77))
    ws_b, sv_b = ops.train_unit_sizes(_lib.UNIT_RCAB, 256, *shape)
    assert (ws_b, sv_b) == (l.balf_rcab_train_workspace_bytes(*shape), l.balf_rcab_train_saved_bytes(*shape))
    outs = []
    for c_arg in ((), (256,)):
        fwd = l.balf_rcab_train_forward_c if c_arg else l.balf_rcab_train_forward
        bwd = l.balf_rcab_train_backward_c if c_arg else l.balf_rcab_train_backward
        ws = torch.full((ws_b,), NAN_BYTE, dtype=torch.uint8, device=DEV)
        sv = torch.full((sv_b,), NAN_BYTE, dtype=torch.uint8, device=DEV)
        x2, dy = torch.empty_like(y), torch.empty_like(y)
        grads = [torch.empty_like(p[k]) for k in R.PARAMS]
        ptr = lambda t: t.data_ptr()                               # noqa: E731
        assert fwd(ptr(y), ptr(r), *[ptr(p[k]) for k in R.PARAMS], *shape, *c_arg, ptr(x2), ptr(sv), ptr(ws), ws_b, None) == 0
        assert bwd(ptr(g), ptr(y), *[ptr(p[k]) for k in ("ln_g", "wc1", "wc2", "ws0", "ws2")], ptr(sv), *shape, *c_arg,
                   *[ptr(t) for t in grads], ptr(dy), ptr(ws), ws_b, None) == 0
        torch.cuda.synchronize()
        outs.append([x2, dy] + grads)
    assert all(bits_equal(a, b) for a, b in zip(*outs))

    x0, p, g = (T.to_device(t, DEV) for t in G.sweep_case(shape, 78))
    ws_b, sv_b = ops.train_unit_sizes(_lib.UNIT_GMLP, 256, *shape)
    assert (ws_b, sv_b) == (l.balf_gmlp_train_workspace_bytes(*shape), l.balf_gmlp_train_saved_bytes(*shape))
    params = [p[k] for k in G.PARAMS]
    outs = []
    for c_arg in ((), (256,)):
        fwd = l.balf_gmlp_train_forward_c if c_arg else l.balf_gmlp_train_forward
        bwd = l.balf_gmlp_train_backward_c if c_arg else l.balf_gmlp_train_backward
        ws = torch.full((ws_b,), NAN_BYTE, dtype=torch.uint8, device=DEV)
        sv = torch.full((sv_b,), NAN_BYTE, dtype=torch.uint8, device=DEV)
        y, dx0 = torch.empty_like(x0), torch.empty_like(x0)
        grads = [torch.empty_like(t) for t in params]
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])       # noqa: E731
        assert fwd(x0.data_ptr(), arr(params), *shape, *c_arg, y.data_ptr(), sv.data_ptr(), ws.data_ptr(), ws_b, None) == 0
        assert bwd(g.data_ptr(), x0.data_ptr(), arr(params), sv.data_ptr(), *shape, *c_arg, arr(grads), dx0.data_ptr(),
                   ws.data_ptr(), ws_b, None) == 0
        torch.cuda.synchronize()
        outs.append([y, dx0] + grads)
    assert all(bits_equal(a, b) for a, b in zip(*outs))
    # a width the units do not take: refused by its code, nothing launched
    assert l.balf_rcab_train_forward_c(*([x0.data_ptr()] * 12), *shape, 64, x0.data_ptr(), sv.data_ptr(), ws.data_ptr(), ws_b, None) == -2
    assert l.balf_gmlp_train_forward_c(x0.data_ptr(), arr(params), *shape, 192, y.data_ptr(), sv.data_ptr(), ws.data_ptr(), ws_b,
                                       None) == -2


# ---- the pool: exact -------------------------------------------------------------------------------------------------------------
# output maps (B, Ho, Wo): one pixel; odd sizes; (2,8,8); and "stride": the smallest odd square map whose Ho * Wo * C / 4 quads
# exceed the 2048 x 256 threads of the kernel's grid, so that some threads take a second round of the grid-stride loop
POOL_MAPS = ((1, 1, 1), (3, 3, 5), (2, 8, 8), "stride")
POOL_STRIDE_MAPS = {32: (1, 257, 257), 128: (1, 129, 129), 256: (1, 91, 91)}


@pytest.mark.parametrize("c", (32, 128, 256))
@pytest.mark.parametrize("shape", POOL_MAPS)
def test_pool_is_torchs_max_pool2d_bit_for_bit(shape, c):
    past_stride = shape == "stride"
    if past_stride:
        shape = POOL_STRIDE_MAPS[c]
        assert shape[1] * shape[2] * (c // 4) > 2048 * 256 >= (shape[1] - 2) * (shape[2] - 2) * (c // 4)
    cases = Sc.pool_cases(shape, c, 300 + c + sum(shape))
    if past_stride:
        cases = {k: cases[k] for k in ("random", "nan3")}                      # the large map: the index arithmetic, two inputs
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(shape + (c,), generator=gen)
    for name, x in cases.items():
        want_out, want_which, want_dx = Sc.pool_reference(x, g)
        f = ops.pool_train_forward(x.to(DEV))
        assert f.out.shape == want_out.shape and f.which.dtype == torch.uint8 and f.which.shape == want_which.shape
        assert bits_equal(f.out.cpu(), want_out), (name, "out")
        assert torch.equal(f.which.cpu(), want_which), (name, "which")
        # dx arrives pre-filled with NaN: an element that the backward does not write shows
        dx = torch.full(x.shape, float("nan"), device=DEV)
        ops.launch("balf_pool_train_backward", DEV, g.to(DEV), f.which, shape[0], 2 * shape[1], 2 * shape[2], c, dx)
        assert bits_equal(dx.cpu(), want_dx), (name, "dx")
        assert bits_equal(ops.pool_train_backward(g.to(DEV), f.which).cpu(), want_dx), (name, "dx through ops")


def test_pool_argument_errors():
    l = ops.lib()
    x = torch.zeros((1, 4, 6, 8), device=DEV)
    out, which = torch.zeros((1, 2, 3, 8), device=DEV), torch.zeros((1, 2, 3, 8), dtype=torch.uint8, device=DEV)
    ptr = lambda t: t.data_ptr()                                   # noqa: E731
    f, b = l.balf_pool_train_forward, l.balf_pool_train_backward
    assert f(ptr(x), 1, 4, 6, 8, ptr(out), ptr(which), None) == 0 and b(ptr(out), ptr(which), 1, 4, 6, 8, ptr(x), None) == 0
    for dims in ((1, 3, 6, 8), (1, 4, 5, 8), (1, 4, 6, 6), (1, 4, 6, 260), (1, 4, 6, 0), (1, 4096, 4098, 8)):
        assert f(ptr(x), *dims, ptr(out), ptr(which), None) == -2 and b(ptr(out), ptr(which), *dims, ptr(x), None) == -2, dims
    for dims in ((0, 4, 6, 8), (65536, 4, 6, 8), (1, 0, 6, 8), (1, 4, -2, 8)):
        assert f(ptr(x), *dims, ptr(out), ptr(which), None) == -1 and b(ptr(out), ptr(which), *dims, ptr(x), None) == -1, dims
    assert f(None, 1, 4, 6, 8, ptr(out), ptr(which), None) == -1 and f(ptr(x), 1, 4, 6, 8, None, ptr(which), None) == -1
    assert f(ptr(x) + 4, 1, 4, 6, 8, ptr(out), ptr(which), None) == -1 and f(ptr(x), 1, 4, 6, 8, ptr(out), ptr(which) + 4, None) == -1
    assert b(ptr(out), None, 1, 4, 6, 8, ptr(x), None) == -1 and b(ptr(out) + 8, ptr(which), 1, 4, 6, 8, ptr(x), None) == -1
    torch.cuda.synchronize()
    with pytest.raises(ops.BalfHipError, match="even"):
        ops.pool_train_forward(torch.zeros((1, 3, 4, 8), device=DEV))
    with pytest.raises(ops.BalfHipError, match="multiple of 4"):
        ops.pool_train_forward(torch.zeros((1, 4, 4, 6), device=DEV))
    with pytest.raises(ops.BalfHipError, match="which"):
        ops.pool_train_backward(out, which.float())


def test_graph_capture_of_the_pool_and_the_rcab():
    """Forward and backward of the pool and of the block at C = 128, captured once and replayed on new inputs."""
    shape = (2, 6, 10)
    cases = [R.sweep_case(shape, 60 + i, c=C3) for i in range(3)]
    y, r, p, g = cases[0]
    static = {"y": y.to(DEV), "r": r.to(DEV), "g": g.to(DEV), **{k: v.to(DEV) for k, v in p.items()}}
    gp = torch.randn((2, 3, 5, C3), generator=torch.Generator().manual_seed(9)).to(DEV)

    def step():
        s = static
        f = ops.rcab_train_forward(s["y"], s["r"], [s[k] for k in R.PARAMS], channels=C3)
        pooled = ops.pool_train_forward(f.x2)
        dpre = ops.pool_train_backward(gp, pooled.which)
        b = ops.rcab_train_backward(s["g"], s["y"], s["ln_g"], s["wc1"], s["wc2"], s["ws0"], s["ws2"], f.saved, want_dy=True,
                                    channels=C3)
        return (f.x2,) + tuple(b) + (pooled.out, pooled.which, dpre)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        outs = step()
    for y, r, p, g in cases[1:]:
        for k, v in dict(p, y=y, r=r, g=g).items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run_rcab(y, r, p, g)
        for a, k in zip(outs, R.GATED):
            assert bits_equal(a, want[k]), k
        want_out, want_which, want_dx = Sc.pool_reference(want["x2"], gp)
        assert bits_equal(outs[-3].cpu(), want_out) and torch.equal(outs[-2].cpu(), want_which) and bits_equal(outs[-1].cpu(), want_dx)


# ---- the whole stage -------------------------------------------------------------------------------------------------------------
def synthetic_model(seed, precision):
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(seed))
    model.precision = precision
    return model.eval().to(DEV)


def test_stage3_backward_against_the_fixture(fx):
    """TrainableStage3 of synth.synthetic_state_dict(0) on the stored x2s (the stage-3 map is 16 x 16, stage 4's 8 x 8) with the
    dlogits of the reference's loss: one backward(), all 38 gradients of stage 3 and x2s.grad against the restatement."""
    x2s, sp, dlogits = Sc.stage_inputs(fx)
    res = Sc.stage64(x2s, sp, dlogits)
    stage = TrainableStage3.from_model(synthetic_model(0, "fp32"))
    params = list(stage.parameters())
    own = dict(stage.down3.named_parameters())
    assert tuple(own) == Sc.STAGE3_NAMES and len(params) == 82
    assert sum(p.numel() for p in own.values()) == 224544 and sum(p.numel() for p in params) == 1173923
    xd = x2s.to(DEV).requires_grad_()
    out = stage(xd, want_prob=False)
    out["logits"].backward(dlogits.to(DEV))
    torch.cuda.synchronize()
    got = {"d:" + n: own[n].grad for n in Sc.STAGE3_NAMES}
    got["dx2s"] = xd.grad
    assert all(v is not None for v in got.values())
    worst = check_against(got, res, fx, "stage", "stage3", Sc.STAGE_GATED)
    print(f"stage3: largest err {worst:.3e}; logits {Sc.err(out['logits'], res['logits'], 1.0):.3e} absolute")
    # the pool chose what the restatement chose: its gap is POOL_FACTOR float32 movements of pre wide
    assert float(fx["stage.pool_gap"]) > Sc.POOL_FACTOR * float(fx["stage.pool_moved"])


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
def test_stage2_level_and_eval_logits(precision):
    """encode(level="stage2") is the stage view of stage 2 -- whole, in chunks and in halves the same bits --, and the module in
    eval() on it gives the model's logits."""
    model = synthetic_model(3, precision)
    gen = torch.Generator().manual_seed(12)
    x = torch.rand((4, 3, 64, 128), generator=gen).to(DEV)
    x2s = model.encode(x, level="stage2")
    assert model.effective_precision == precision
    assert x2s.shape == (4, 16, 32, 64) and x2s.dtype == torch.float32 and not x2s.requires_grad and x2s.is_contiguous()
    assert bits_equal(x2s, model.encode(x, chunk=1, level="stage2")) and bits_equal(x2s, model.encode(x, chunk=3, level="stage2"))
    assert bits_equal(x2s[:2], model.encode(x[:2], level="stage2")) and bits_equal(x2s[2:], model.encode(x[2:], level="stage2"))
    with pytest.raises(ValueError, match="'stage2'"):
        model.encode(x, level="stage1")
    stage = TrainableStage3.from_model(model).eval()
    assert not stage.stage4.mixer.tail.head.training
    got, want = stage(x2s)["logits"], model(x)["logits"]
    print(precision, "eval logits differ by", float((got - want).abs().max()))
    assert float((got - want).abs().max()) <= LOGIT_TOL


def test_train_stage3_end_to_end():
    """The chunk of test_train_stage4_end_to_end: one pair of 64 x 64 windows with dense labels, presented six times to Adam(lr =
    1e-3) from build_optimizer (82 tensors: two launches of the fused step), here through stages 3-4 and the head."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    chunk = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(chunk) == 1 and chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = synthetic_model(2, "fp32")
    x = chunk[0][0]
    before = train_utils.check_val_anchor_loss(chunk, model, DEV)
    stage = TrainableStage3.from_model(model)
    assert stage.encode_level == "stage2" and len(list(stage.parameters())) == 82
    key = model._weights_key(DEV)
    opt = train_utils.build_optimizer(stage.parameters(), {"name": "adam", "lr": 1e-3, "weight_decay": 0.0})
    gpu = [train_utils.train_head(chunk, model, stage, opt, DEV, noise=False) for _ in range(6)]
    assert model._weights_key(DEV) == key                       # the model was not touched: no re-pack while training
    assert int(stage.stage4.mixer.tail.head.norm.num_batches_tracked) == 12
    feats = [(model.encode(b[0], level="stage2").cpu(), model.encode(b[1], level="stage2").cpu(), b[2].cpu(), b[3].cpu()) for b in chunk]
    sd = synth.synthetic_state_dict(2)
    cpu = Sc.train64(feats, Sc.stage_params(sd), 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; GPU", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    print("largest difference", max(abs(a - b) for a, b in zip(gpu, cpu)))
    # The tolerance of test_train_stage4_end_to_end.  Adam's update is a continuous function of the gradients, which agree to
    # ~1e-6 of their scales through stage 3 as through stage 4 (case ``stage`` of the fixture: d_T <= 6.3e-7), the float32 loss
    # itself carries ~1e-7 of a value of a few units, and the measured difference is printed above.
    assert max(abs(a - b) for a, b in zip(gpu, cpu)) <= 5e-5
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    w0 = stage.down3.conv._modules["0"].weight.detach().cpu()
    assert float((w0 - sd["down3.conv.0.weight"]).abs().max()) > 1e-4                  # stage 3 itself moved
    x2s = model.encode(x, level="stage2")
    stage.commit(model)
    assert model._weights_key(DEV) != key
    assert bits_equal(model.state_dict()["down3.conv.0.weight"], stage.down3.conv._modules["0"].weight.detach())
    assert bits_equal(model.encode(x, level="stage2"), x2s)     # stages 1-2 did not move
    got, want = model.eval()(x)["logits"], stage.eval()(x2s)["logits"]
    assert float((got - want).abs().max()) <= LOGIT_TOL
    after = train_utils.check_val_anchor_loss(chunk, model, DEV)
    print(f"check_val_anchor_loss before {before:.4f} after {after:.4f}")
    assert after < before
