"""Stage 4's channel-attention block in training form on the GPU (balf_rcab_train_forward / balf_rcab_train_backward /
balf_forward_rcab_inputs, ops.rcab_*, model.tail_train.TrainableTail, MLP_MA_DECODER.encode(level="rcab"),
utils.train_utils.train_head) against tests/golden/rcab_train.npz -- the reference's own modules and autograd, recorded by
tests/golden/make_rcab_train_golden.py -- and against the float64 restatement of tests/rcab_train_common.py.  Every output T is
gated by err(T) = max |T - T64| / S_T <= tol_T = max(4 * d_T, 1.1e-6), d_T the reference's own float32 distance from the
restatement (rcab_train_common.restate64 defines the scales S_T)."""
import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.tail_train import TrainableTail
from balf_amd.utils import synth, train_utils
from oracle import oracle
from tests import head_train_common as H
from tests import pair_synth_common as S
from tests import rcab_train_common as R
from tests import train_common as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGIT_TOL = 2e-3                # the gate tests/test_forward_gpu.py applies to the logits of the forward
STAGE_REL = 2e-5                # the gate of tests/test_stage_parity_gpu.py
# one pixel per image (dm / 1, the SE mean of one value); N below one GEMM tile and N no multiple of 64; S = 9 slabs at N = 2304;
# images of 851 pixels, which start and end inside the 64-row blocks of the sums over all pixels; N = 4096
SWEEP = ((1, 1, 2), (2, 1, 1), (1, 3, 5), (1, 8, 8), (1, 5, 13), (2, 7, 9), (3, 24, 24), (2, 23, 37), (4, 32, 32))
# Where the slice geometry changes (tests/test_train_geometry_host.py asserts each figure).  N = 16899: 512 rows per K slice, S = 34
# with a last slice of 3 rows, a last column block of 3 rows.  (2, 257, 257), N = 132098: 2304 rows per slice, S = 58, column blocks
# of 144 rows, PC = 918 with a last block of 50 rows; an image of 66049 pixels is summed in PI = 1017 blocks of 65 rows with a last
# block of 9 rows, and image 1 begins inside column block 458.  Cases, margin checks and restatement on the device.
LARGE = T.LARGE_SHAPES["rcab"]
NAN_BYTE = 0xFF                # a buffer of these bytes reads as NaN in float32 and in float64


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def poison_workspace(shape):
    """Fill the cached workspace of this stream with NaN bytes: a stale word that is read shows in the results."""
    ops._workspace("rcab_train", DEV, ops.lib().balf_rcab_train_workspace_bytes(*shape)).fill_(NAN_BYTE)


def run(y, r, p, g, want_dy=True, poison=True):
    """One forward and one backward through ops on the device -> dict of device tensors (GATED).  ``poison``: the workspace,
    ``saved`` and dy hold NaN bytes before the calls (the other outputs are fresh ``torch.empty`` tensors of ops)."""
    shape = tuple(y.shape[:3])
    d = [p[k].to(DEV) for k in R.PARAMS]
    yd, rd, gd = y.to(DEV), r.to(DEV), g.to(DEV)
    saved = None
    if poison:
        poison_workspace(shape)
        saved = torch.full((ops.lib().balf_rcab_train_saved_bytes(*shape),), NAN_BYTE, dtype=torch.uint8, device=DEV)
    f = ops.rcab_train_forward(yd, rd, d, saved=saved)
    if poison:
        poison_workspace(shape)
    dy = want_dy
    if want_dy is True and poison:
        dy = torch.full(yd.shape, float("nan"), device=DEV)
    ln_g, _, wc1, _, wc2, _, ws0, _, ws2, _ = d
    b = ops.rcab_train_backward(gd, yd, ln_g, wc1, wc2, ws0, ws2, f.saved, want_dy=dy)
    torch.cuda.synchronize()
    out = {"x2": f.x2}
    out.update({k: getattr(b, k) for k in R.GRADS})
    return out


def check_against(out, res, fx, what, names=R.GATED):
    errs = {k: R.err(out[k], res[k], res["S"][k]) for k in names if out.get(k) is not None}
    print(what, " ".join(f"{k} {e:.2e}" for k, e in errs.items()))                # every figure before any assertion
    bad = {k: (e, float(fx[f"tol_{k}"])) for k, e in errs.items() if not (np.isfinite(e) and e <= float(fx[f"tol_{k}"]))}
    assert not bad, (what, bad)
    return errs


@pytest.mark.parametrize("name", R.FIXTURE_CASES)
def test_fixture_parity(fx, name):
    y, r, p, g = R.fixture_case(fx, name)
    res = R.restate64(y, r, p, g)
    out = run(y, r, p, g)
    assert all(out[k] is not None for k in R.GATED)             # all twelve
    check_against(out, res, fx, name)
    if name == "edges":
        c = R.EDGES_LN_G0                                       # ln_g = 0: n says nothing about xhat there, dln_g does
        assert float(res["dln_g"][c].abs()) > 1e-3 * res["S"]["dln_g"]
        assert abs(float(out["dln_g"][c]) - float(res["dln_g"][c])) <= float(fx["tol_dln_g"]) * res["S"]["dln_g"]
        # h == 0 exactly on channels 0..7 of the constant row: the slope is 0.2 there.  dbc1 of those channels tells: the sum with
        # that element at slope 1 lies far outside the gate
        da = res["dt"] @ p["wc2"].double()
        wrong = (da * torch.where(res["h"] >= 0, 1.0, R.SLOPE)).sum(0)
        tol = float(fx["tol_dbc1"]) * res["S"]["dbc1"]
        got = out["dbc1"].double().cpu()
        assert float((got[:R.EDGES_H0] - res["dbc1"][:R.EDGES_H0]).abs().max()) <= tol \
            < 0.1 * float((wrong[:R.EDGES_H0] - res["dbc1"][:R.EDGES_H0]).abs().min())
        # the SE unit with e == 0 exactly passes no gradient: its row of dws0 and its dbs0 are exact zeros
        assert bool((out["dws0"][R.EDGES_E0] == 0).all()) and float(out["dbs0"][R.EDGES_E0]) == 0.0
        # the constant row: xhat = 0 exactly, so dy = g + rstd * (u - mean u) there, with rstd = 1 / sqrt(eps)
        at = R.EDGES_CONST_ROW
        e = float((out["dy"][at].double().cpu() - res["dy"][at]).abs().max()) / res["S"]["dy"]
        assert e <= float(fx["tol_dy"]), e


@pytest.mark.parametrize("name", R.FIXTURE_CASES)
def test_autograd_path_against_the_reference(fx, name):
    """Through TrainableTail and its head: the ten gradients of the block, the six of the head and y.grad from ONE backward().
    Case ``model`` starts from the seeded dlogits, as the recorder did, so that dx2 is the GPU head's own; case ``edges`` has no
    head in the recording and sends its dx2 into the block."""
    y, r, p, g = R.fixture_case(fx, name)
    res = R.restate64(y, r, p, g)
    tail = TrainableTail().to(DEV)
    with torch.no_grad():
        for k, t in zip(R.PARAMS, tail.rcab_parameters()):
            t.copy_(p[k])
    yd = y.to(DEV).requires_grad_()
    if name == "model":
        _, _, dlogits, (hp, running) = R.model_inputs()
        head = tail.head
        with torch.no_grad():
            for k, t in zip(H.PARAMS, (head.conv2.weight, head.conv2.bias, head.dense.weight, head.dense.bias, head.norm.weight,
                                       head.norm.bias)):
                t.copy_(hp[k])
            head.norm.running_mean.copy_(running[0])
            head.norm.running_var.copy_(running[1])
        out = tail((yd, r.to(DEV)))
        assert out["logits"].grad_fn is not None and not out["prob"].requires_grad
        (out["logits"] * dlogits.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        hfx = H.fixture()
        hres = H.restate64(torch.from_numpy(hfx["model.x2"]), hp, dlogits, running=running)
        hgot = {"logits": out["logits"], "dw2": head.conv2.weight.grad, "db2": head.conv2.bias.grad, "dwd": head.dense.weight.grad,
                "dbd": head.dense.bias.grad, "dgamma": head.norm.weight.grad, "dbeta": head.norm.bias.grad}
        bad = {}
        for k, v in hgot.items():                               # the head's six (and its logits), on the x2 this block produced
            e = H.err(v, torch.from_numpy(hfx[f"model.{k}"]), hres["S"][k])
            print("head", k, f"{e:.2e}")
            if not e <= float(hfx[f"tol_{k}"]):
                bad[k] = e
        assert not bad, bad
        assert int(head.norm.num_batches_tracked) == 1
    else:
        x2 = _rcab_apply(tail, yd, r.to(DEV))
        assert x2.grad_fn is not None
        x2.backward(g.to(DEV))
        torch.cuda.synchronize()
    got = {"d" + k: t.grad for k, t in zip(R.PARAMS, tail.rcab_parameters())}
    got["dy"] = yd.grad
    bad = {}
    for k in R.GRADS:                                           # against the recorded REFERENCE, in the restatement's scales
        ref, mine = R.recorded(fx, name, k, got[k].detach().cpu())
        e = R.err(mine, ref, res["S"][k])
        print(name, k, f"{e:.2e}")
        if not e <= float(fx[f"tol_{k}"]):
            bad[k] = e
    assert not bad, bad
    if name == "edges":
        # no gradient wanted for y: dy is not asked for, the parameter gradients are the same bits
        tail.zero_grad()
        _rcab_apply(tail, y.to(DEV), r.to(DEV)).backward(g.to(DEV))
        for k, t in zip(R.PARAMS, tail.rcab_parameters()):
            assert bits_equal(t.grad, got["d" + k]), k


def _rcab_apply(tail, y, r):
    from balf_amd.model.tail_train import _RcabTrain
    return _RcabTrain.apply(y, r, *tail.rcab_parameters())


_LARGEST = {}


def largest():
    """The last case of LARGE on the device and its first run, made once -> (case, outputs)."""
    if not _LARGEST:
        shape = LARGE[-1]
        c = R.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        _LARGEST.update(case=c, out=run(*c))
    return _LARGEST["case"], _LARGEST["out"]


@pytest.mark.parametrize("shape", SWEEP + LARGE, ids=lambda s: "x".join(map(str, s)))
def test_shape_sweep(fx, shape):
    if shape not in LARGE:
        y, r, p, g = R.sweep_case(shape, 7 + shape[1] * 100 + shape[2])
        res = R.restate64(y, r, p, g)
        check_against(run(y, r, p, g), res, fx, str(shape))
        return
    # the same gates with the case (its margin checks too), the float64 restatement and the float32 composition on the device
    if shape == LARGE[-1]:
        (y, r, p, g), out = largest()
    else:
        y, r, p, g = R.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        out = run(y, r, p, g)
    res = R.restate64(y, r, p, g)
    x2, grads = R.compose_f32(y, r, p, g)
    T.composition_figures(str(shape), dict(grads, x2=x2), res, R.GATED)
    check_against(out, res, fx, str(shape))


def test_largest_shape_gives_the_same_bits_again_and_without_dy():
    """The fixed summation order over PC = 918 column blocks of 144 rows, PI = 1017 image blocks of 65 rows and S = 58 slabs; and
    ln_bwd_kernel<false>, the instantiation without dy, at that block height: the parameter gradients are the same bits."""
    c, a = largest()
    b = run(*c)
    for k in R.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k
    del b
    lean = run(*c, want_dy=False)
    assert lean["dy"] is None
    for k in R.GATED[:-1]:
        assert bits_equal(a[k], lean[k]), k


def test_bitwise_repeatability():
    c = R.sweep_case((2, 23, 37), 50)
    a, b = run(*c), run(*c)
    for k in R.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_independence_of_requests():
    c = R.sweep_case((2, 23, 37), 51)
    full = run(*c)
    lean = run(*c, want_dy=False)
    assert lean["dy"] is None
    for k in R.GATED[:-1]:
        assert bits_equal(full[k], lean[k]), k
    # dy into a view that starts 4 bytes into its buffer: the 4-byte stores instead of the 16-byte ones, same bits, nothing outside
    buf = torch.full((c[0].numel() + 2,), float("nan"), device=DEV)
    view = buf[1:-1].view(c[0].shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    off = run(*c, want_dy=view)
    assert off["dy"] is view and bits_equal(view, full["dy"]) and bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))
    for k in R.GATED[:-1]:
        assert bits_equal(full[k], off[k]), k


def test_graph_capture():
    shape = (2, 7, 9)
    cases = [R.sweep_case(shape, 60 + i) for i in range(3)]
    y, r, p, g = cases[0]
    static = {"y": y.to(DEV), "r": r.to(DEV), "g": g.to(DEV), **{k: v.to(DEV) for k, v in p.items()}}

    def step():
        s = static
        f = ops.rcab_train_forward(s["y"], s["r"], [s[k] for k in R.PARAMS])
        b = ops.rcab_train_backward(s["g"], s["y"], s["ln_g"], s["wc1"], s["wc2"], s["ws0"], s["ws2"], f.saved, want_dy=True)
        return (f.x2,) + tuple(b)

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
        want = run(y, r, p, g, poison=False)
        for a, k in zip(outs, R.GATED):
            assert bits_equal(a, want[k]), k


def synthetic_model(seed, precision):
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(seed))
    model.precision = precision
    return model.eval().to(DEV)


def test_eval_mode(fx):
    y, r, p, g = R.fixture_case(fx, "edges")
    res = R.restate64(y, r, p)
    tail = TrainableTail().to(DEV)
    with torch.no_grad():
        for k, t in zip(R.PARAMS, tail.rcab_parameters()):
            t.copy_(p[k])
    tail.eval()
    assert not tail.head.training
    poison_workspace(R.EDGES_SHAPE)
    out = tail((y.to(DEV).requires_grad_(), r.to(DEV)))
    assert out["logits"].grad_fn is None and int(tail.head.norm.num_batches_tracked) == 0
    # the same arithmetic as the training forward: the eval head on the ops' x2 gives the same bits
    x2 = ops.rcab_train_forward(y.to(DEV), r.to(DEV), [t.detach() for t in tail.rcab_parameters()]).x2
    check_against({"x2": x2}, res, fx, "eval", names=("x2",))
    assert bits_equal(out["logits"], tail.head(x2)["logits"])
    assert tail((y.to(DEV), r.to(DEV)), want_prob=False)["prob"] is None


_ORACLE = {}


def oracle_taps(shape):
    """The seeded image of a shape and the oracle's (x1, x1 + x0) of stage 4 in float64, computed once per shape."""
    if shape not in _ORACLE:
        g = torch.Generator().manual_seed(11 + shape[2])
        x = torch.rand((shape[0], 3, shape[1], shape[2]), generator=g)
        taps = {}
        oracle.detector_forward(oracle.cast_state(synth.synthetic_state_dict(3), torch.float64), x.double(), taps=taps)
        x1, x2, t, s = taps["down4.x1"], taps["down4.x2"], taps["down4.t"], taps["down4.s"]
        _ORACLE[shape] = (x, x1, x2 - t * s[:, None, None, :])   # x2 = t s + x1 + x0
    return _ORACLE[shape]


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
@pytest.mark.parametrize("shape", ((3, 128, 192), (1, 64, 448)), ids=("3x128x192", "1x64x448"))
def test_encode_rcab_against_the_oracle(precision, shape):
    """(y, r) against the oracle's down4.x1 and x1 + x0 taps, by the measure and gate of tests/test_stage_parity_gpu.py."""
    model = synthetic_model(3, precision)
    x, x1, want_r = oracle_taps(shape)
    before = model.encode(x.to(DEV))
    y, r = model.encode(x.to(DEV), level="rcab")
    assert y.shape == r.shape == (shape[0], shape[1] // 8, shape[2] // 8, 256) and y.dtype == torch.float32 and not y.requires_grad
    for name, got, want in (("y", y, x1), ("r", r, want_r)):
        rel = float((got.double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
        print(precision, shape, name, f"rel {rel:.2e}")
        assert rel < STAGE_REL, (name, rel)
    assert bits_equal(model.encode(x.to(DEV)), before)          # nothing of the forward's state was changed


def test_encode_rcab_in_chunks_is_the_concatenation():
    model = synthetic_model(3, "fp32")
    g = torch.Generator().manual_seed(10)
    x = torch.rand((3, 3, 64, 128), generator=g).to(DEV)
    whole = model.encode(x, level="rcab")
    parts = [model.encode(x[i:i + 1], level="rcab") for i in range(3)]
    halves = model.encode(x, chunk=2, level="rcab")
    for k in range(2):
        assert bits_equal(whole[k], torch.cat([p[k] for p in parts])) and bits_equal(halves[k], whole[k])
    with pytest.raises(ValueError):
        model.encode(x, level="x1")


def test_train_tail_end_to_end():
    """The chunk of tests/test_head_train_gpu.py: one pair of 64 x 64 windows with dense labels, presented six times to
    Adam(lr = 1e-3), here through the block and the head."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    chunk = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(chunk) == 1 and chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = synthetic_model(2, "fp32")
    x = chunk[0][0]
    before = train_utils.check_val_anchor_loss(chunk, model, DEV)
    tail = TrainableTail.from_model(model)
    assert tail.encode_level == "rcab"
    key = model._weights_key(DEV)
    opt = torch.optim.Adam(tail.parameters(), lr=1e-3)
    gpu = [train_utils.train_head(chunk, model, tail, opt, DEV, noise=False) for _ in range(6)]
    assert model._weights_key(DEV) == key                       # the model was not touched: no re-pack while training
    assert int(tail.head.norm.num_batches_tracked) == 12
    # the same six presentations in float64 on the CPU, from the same features
    cpu_of = lambda f: tuple(t.cpu() for t in f)                # noqa: E731
    feats = [(cpu_of(model.encode(b[0], level="rcab")), cpu_of(model.encode(b[1], level="rcab")), b[2].cpu(), b[3].cpu())
             for b in chunk]
    sd = synth.synthetic_state_dict(2)
    hp, running = H.params_of(sd)
    cpu = R.train64(feats, R.params_of(sd), hp, running, 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; GPU", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    # the fourth decimal, the last digit the head's test prints: Adam's update is a continuous function of the gradients, which
    # agree to ~1e-6 of their scales, and the float32 loss itself carries ~1e-7 of a value of a few units
    assert max(abs(a - b) for a, b in zip(gpu, cpu)) <= 5e-5
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    tail.commit(model)
    assert model._weights_key(DEV) != key
    got, want = model.eval()(x)["logits"], tail.eval()(model.encode(x, level="rcab"))["logits"]
    assert float((got - want).abs().max()) <= LOGIT_TOL
    after = train_utils.check_val_anchor_loss(chunk, model, DEV)
    print(f"check_val_anchor_loss before {before:.4f} after {after:.4f}")
    assert after < before
