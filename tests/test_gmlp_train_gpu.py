"""Stage 4's multi-axis gated-MLP layer in training form on the GPU (balf_gmlp_train_forward / balf_gmlp_train_backward /
balf_forward_gmlp_input, ops.gmlp_*, model.mixer_train.TrainableMixerTail, MLP_MA_DECODER.encode(level="gmlp"),
utils.train_utils.train_head) against tests/golden/gmlp_train.npz -- the reference's own modules and autograd, recorded by
tests/golden/make_gmlp_train_golden.py -- and against the float64 restatement of tests/gmlp_train_common.py.  Every output T is
gated by err(T) = max |T - T64| / S_T <= tol_T = max(4 * d_T, 1.1e-6), d_T the reference's own float32 distance from the
restatement (gmlp_train_common.restate64 defines the scales S_T)."""
import ctypes as C

import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.mixer_train import TrainableMixerTail, _GmlpTrain
from balf_amd.utils import synth, train_utils
from oracle import oracle
from tests import gmlp_train_common as G
from tests import head_train_common as H
from tests import pair_synth_common as S
from tests import rcab_train_common as R
from tests import train_common as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGIT_TOL = 2e-3                # the gate tests/test_forward_gpu.py applies to the logits of the forward
STAGE_REL = 2e-5                # the gate of tests/test_stage_parity_gpu.py
# one group per map; two images; regions of 1 x 2 and 2 x 1 pixels; three images with regions of 2 x 3; N = 960, where the last of
# the 64-row blocks of the column sums is short and several groups share a workgroup of the token-mix backward (960 / 64 = 15
# groups; 272 at the last shape, two per workgroup); N = 17408 = 34 x 512: two 256-pixel chunks per K slice (rows_per_slice
# exceeds 256 from N = 16385 on), every slice and every column block full
SWEEP = ((1, 8, 8), (2, 8, 16), (2, 16, 8), (3, 16, 24), (1, 24, 40), (1, 128, 136))
# Where the slice geometry changes (tests/test_train_geometry_host.py asserts each figure).  (1, 8, 2056), N = 16448: 512 rows per K
# slice, S = 33 with a last slice of 64 rows; 257 groups, two per workgroup of the token-mix backward, PW = 129 with ONE group in the
# last; the grid map's regions are 1 x 257 pixels.  (2, 216, 152), N = 65664: 1280 rows per slice, S = 52, column blocks of 80 rows, PC
# = 821 with a last block of 64 rows; 1026 groups, five per workgroup, PW = 206 with one group in the last.  Cases and restatement on
# the device.
LARGE = T.LARGE_SHAPES["gmlp"]
NAN_BYTE = 0xFF                # a buffer of these bytes reads as NaN in float32 and in float64


@pytest.fixture(scope="module")
def fx():
    return G.fixture()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def poison_workspace(shape):
    """Fill the cached workspace of this stream with NaN bytes: a stale word that is read shows in the results."""
    ops._workspace("gmlp_train", DEV, ops.lib().balf_gmlp_train_workspace_bytes(*shape)).fill_(NAN_BYTE)


def run(x0, p, g, want_dx0=True, poison=True):
    """One forward and one backward through ops on the device -> dict of device tensors (GATED).  ``poison``: the workspace,
    ``saved`` and dx0 hold NaN bytes before the calls (the other outputs are fresh ``torch.empty`` tensors of ops)."""
    shape = tuple(x0.shape[:3])
    d = [p[k].to(DEV) for k in G.PARAMS]
    xd, gd = x0.to(DEV), g.to(DEV)
    saved = None
    if poison:
        poison_workspace(shape)
        saved = torch.full((ops.lib().balf_gmlp_train_saved_bytes(*shape),), NAN_BYTE, dtype=torch.uint8, device=DEV)
    f = ops.gmlp_train_forward(xd, d, saved=saved)
    if poison:
        poison_workspace(shape)
    dx0 = want_dx0
    if want_dx0 is True and poison:
        dx0 = torch.full(xd.shape, float("nan"), device=DEV)
    b = ops.gmlp_train_backward(gd, xd, d, f.saved, want_dx0=dx0)
    torch.cuda.synchronize()
    out = {"y": f.y, "dx0": b.dx0}
    out.update({"d:" + k: t for k, t in zip(G.PARAMS, b.grads)})
    return out


def check_against(out, res, fx, what, names=G.GATED):
    errs = {k: G.err(out[k], res[k], res["S"][k]) for k in names if out.get(k) is not None}
    print(what, " ".join(f"{k} {e:.2e}" for k, e in errs.items()))                # every figure before any assertion
    bad = {k: (e, float(fx[f"tol_{k}"])) for k, e in errs.items() if not (np.isfinite(e) and e <= float(fx[f"tol_{k}"]))}
    assert not bad, (what, bad)
    return errs


_CASES = {}


def case64(fx, name):
    """A fixture case and its float64 restatement, computed once."""
    if name not in _CASES:
        c = G.fixture_case(fx, name)
        _CASES[name] = (c, G.restate64(*c))
    return _CASES[name]


@pytest.mark.parametrize("name", G.FIXTURE_CASES)
def test_fixture_parity(fx, name):
    (x0, p, g), res = case64(fx, name)
    out = run(x0, p, g)
    assert all(out[k] is not None for k in G.GATED)             # all 28
    check_against(out, res, fx, name)
    if name == "edges":
        gl, gu = G.BRANCHES[0]
        bl, bu = G.BRANCHES[1]
        # the gating LayerNorm of the grid branch sees a constant on every pixel: xhat = 0 exactly, its gain's gradient is exactly 0
        assert bool((out[f"d:{gl}.{gu}.norm.weight"] == 0).all())
        # gain = 0 on one channel of the layer's norm: n0 says nothing about xhat there, the gain's gradient does
        k, c = "d:norm.weight", G.EDGES_GAIN0
        assert float(res[k][c].abs()) > 1e-3 * res["S"][k]
        assert abs(float(out[k][c]) - float(res[k][c])) <= float(fx["tol_" + k]) * res["S"][k]
        # the block map's token whose gate is exactly 0 passes nothing on to dense2 and takes da = 0; its row of dWt and its dbt
        # still carry dgated * a
        k = f"d:{bl}.{bu}.dense.bias"
        assert float(res[k][G.EDGES_GATE0].abs()) > 1e-3 * res["S"][k]
        # the constant row of x0: xhat = 0 exactly, so dx0 = dy + rstd * (u - mean u) there, with rstd = 1 / sqrt(eps)
        at = G.EDGES_CONST_ROW
        e = float((out["dx0"][at].double().cpu() - res["dx0"][at]).abs().max()) / res["S"]["dx0"]
        assert e <= float(fx["tol_dx0"]), e


def mixer_with(p):
    m = TrainableMixerTail().to(DEV)
    with torch.no_grad():
        for k, t in zip(G.PARAMS, m.gmlp_parameters()):
            t.copy_(p[k])
    return m


@pytest.mark.parametrize("name", G.FIXTURE_CASES)
def test_autograd_path_against_the_reference(fx, name):
    """Case ``model``: through TrainableMixerTail -- the layer, the channel-attention block and the head -- from the seeded
    dlogits, as the recorder did, with ONE backward(): the 26 gradients of the layer and x0.grad, which must hold all three
    paths into x0 as the reference's does.  Cases ``layout`` and ``edges`` have no tail in the recording and send their dy into
    the layer's Function."""
    (x0, p, g), res = case64(fx, name)
    mixer = mixer_with(p)
    xd = x0.to(DEV).requires_grad_()
    if name == "model":
        _, _, dlogits, (rp, hp, running) = G.model_inputs()
        tail, head = mixer.tail, mixer.tail.head
        with torch.no_grad():
            for k, t in zip(R.PARAMS, tail.rcab_parameters()):
                t.copy_(rp[k])
            for k, t in zip(H.PARAMS, (head.conv2.weight, head.conv2.bias, head.dense.weight, head.dense.bias, head.norm.weight,
                                       head.norm.bias)):
                t.copy_(hp[k])
            head.norm.running_mean.copy_(running[0])
            head.norm.running_var.copy_(running[1])
        out = mixer(xd)
        assert out["logits"].grad_fn is not None and not out["prob"].requires_grad
        (out["logits"] * dlogits.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert int(head.norm.num_batches_tracked) == 1
        # the block's own gradients, on the y this layer produced, against the block's recording
        rfx = R.fixture()
        rres = R.restate64(*R.fixture_case(rfx, "model"))
        for k, t in zip(R.PARAMS, tail.rcab_parameters()):
            ref, mine = R.recorded(rfx, "model", "d" + k, t.grad.detach().cpu())
            e = R.err(mine, ref, rres["S"]["d" + k])
            print("rcab", k, f"{e:.2e}")
            assert e <= float(rfx[f"tol_d{k}"]), (k, e)
    else:
        y = _GmlpTrain.apply(xd, *mixer.gmlp_parameters())
        assert y.grad_fn is not None
        y.backward(g.to(DEV))
        torch.cuda.synchronize()
    got = {"d:" + k: t.grad for k, t in zip(G.PARAMS, mixer.gmlp_parameters())}
    bad = {}
    for k in G.GRADS[:-1]:                                      # against the recorded REFERENCE, in the restatement's scales
        ref, mine = G.recorded(fx, name, k, got[k].detach().cpu())
        e = G.err(mine, ref, res["S"][k])
        print(name, k, f"{e:.2e}")
        if not e <= float(fx[f"tol_{k}"]):
            bad[k] = e
    # x0.grad: the layer's share alone, or (case model) the reference's full gradient -- the layer, its shortcut, the long shortcut
    ref, mine = G.recorded(fx, name, "dx0_full" if name == "model" else "dx0", xd.grad.detach().cpu())
    e = G.err(mine, ref, res["S"]["dx0"])
    print(name, "x0.grad", f"{e:.2e}")
    if not e <= float(fx["tol_dx0"]):
        bad["dx0"] = e
    assert not bad, bad
    if name == "edges":
        # no gradient wanted for x0: dx0 is not asked for, the parameter gradients are the same bits
        mixer.zero_grad()
        _GmlpTrain.apply(x0.to(DEV), *mixer.gmlp_parameters()).backward(g.to(DEV))
        for k, t in zip(G.PARAMS, mixer.gmlp_parameters()):
            assert bits_equal(t.grad, got["d:" + k]), k


_LARGEST = {}


def largest():
    """The last case of LARGE on the device and its first run, made once -> (case, outputs)."""
    if not _LARGEST:
        shape = LARGE[-1]
        c = G.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        _LARGEST.update(case=c, out=run(*c))
    return _LARGEST["case"], _LARGEST["out"]


@pytest.mark.parametrize("shape", SWEEP + LARGE, ids=lambda s: "x".join(map(str, s)))
def test_shape_sweep(fx, shape):
    if shape not in LARGE:
        x0, p, g = G.sweep_case(shape, 7 + shape[1] * 100 + shape[2])
        res = G.restate64(x0, p, g)
        check_against(run(x0, p, g), res, fx, str(shape))
        return
    # the same gates with the case, the float64 restatement and the float32 composition on the device
    if shape == LARGE[-1]:
        (x0, p, g), out = largest()
    else:
        x0, p, g = G.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        out = run(x0, p, g)
    res = G.restate64(x0, p, g)
    y, grads = G.compose_f32(x0, p, g)
    T.composition_figures(str(shape), dict(grads, y=y), res, G.GATED, measure=G.err)
    check_against(out, res, fx, str(shape))


def test_largest_shape_gives_the_same_bits_again_and_without_dx0():
    """The fixed summation order over PC = 821 column blocks of 80 rows, 4 * PW = 824 wave partials of the token mix and S = 52
    slabs; and ln_bwd_kernel<false>, the instantiation without dx0, at that block height: the parameter gradients are the same
    bits."""
    c, a = largest()
    b = run(*c)
    for k in G.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k
    del b
    lean = run(*c, want_dx0=False)
    assert lean["dx0"] is None
    for k in G.GATED[:-1]:
        assert bits_equal(a[k], lean[k]), k


def test_bitwise_repeatability():
    c = G.sweep_case((3, 16, 24), 50)
    a, b = run(*c), run(*c)
    for k in G.GATED:
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_independence_of_requests():
    c = G.sweep_case((3, 16, 24), 51)
    full = run(*c)
    lean = run(*c, want_dx0=False)
    assert lean["dx0"] is None
    for k in G.GATED[:-1]:
        assert bits_equal(full[k], lean[k]), k
    # dx0 into a caller's tensor: the same bits, the same object
    mine = torch.full(c[0].shape, float("nan"), device=DEV)
    into = run(*c, want_dx0=mine)
    assert into["dx0"] is mine and bits_equal(mine, full["dx0"])


def test_graph_capture():
    shape = (2, 8, 16)
    cases = [G.sweep_case(shape, 60 + i) for i in range(3)]
    x0, p, g = cases[0]
    static = {"x0": x0.to(DEV), "g": g.to(DEV), **{k: v.to(DEV) for k, v in p.items()}}

    def step():
        s = static
        params = [s[k] for k in G.PARAMS]
        f = ops.gmlp_train_forward(s["x0"], params)
        b = ops.gmlp_train_backward(s["g"], s["x0"], params, f.saved, want_dx0=True)
        return (f.y,) + tuple(b.grads) + (b.dx0,)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        outs = step()
    for x0, p, g in cases[1:]:
        for k, v in dict(p, x0=x0, g=g).items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run(x0, p, g, poison=False)
        for a, k in zip(outs, G.GATED):
            assert bits_equal(a, want[k]), k


def synthetic_model(seed, precision):
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(seed))
    model.precision = precision
    return model.eval().to(DEV)


def test_eval_mode(fx):
    (x0, p, g), res = case64(fx, "edges")
    mixer = mixer_with(p)
    mixer.eval()
    assert not mixer.tail.training and not mixer.tail.head.training
    poison_workspace(G.EDGES_SHAPE)
    out = mixer(x0.to(DEV).requires_grad_())
    assert out["logits"].grad_fn is None and int(mixer.tail.head.norm.num_batches_tracked) == 0
    # the same arithmetic as the training forward: the eval tail on the ops' y gives the same bits
    y = ops.gmlp_train_forward(x0.to(DEV), [t.detach() for t in mixer.gmlp_parameters()]).y
    check_against({"y": y}, res, fx, "eval", names=("y",))
    assert bits_equal(out["logits"], mixer.tail((y, y + x0.to(DEV)))["logits"])
    assert mixer(x0.to(DEV), want_prob=False)["prob"] is None


_ORACLE = {}


def oracle_x0(shape):
    """The seeded image of a shape and the oracle's x0 of stage 4 in float64, computed once per shape: x2 = t s + x1 + x0."""
    if shape not in _ORACLE:
        g = torch.Generator().manual_seed(11 + shape[2])
        x = torch.rand((shape[0], 3, shape[1], shape[2]), generator=g)
        taps = {}
        oracle.detector_forward(oracle.cast_state(synth.synthetic_state_dict(3), torch.float64), x.double(), taps=taps)
        x1, x2, t, s = taps["down4.x1"], taps["down4.x2"], taps["down4.t"], taps["down4.s"]
        _ORACLE[shape] = (x, x2 - t * s[:, None, None, :] - x1)
    return _ORACLE[shape]


@pytest.mark.parametrize("precision", ("fp32", "fp16"))
@pytest.mark.parametrize("shape", ((3, 128, 192), (1, 64, 448)), ids=("3x128x192", "1x64x448"))
def test_encode_gmlp_against_the_oracle(precision, shape):
    """x0 against the oracle's, by the measure and gate of tests/test_stage_parity_gpu.py; and it is the x0 of level "rcab"."""
    model = synthetic_model(3, precision)
    x, want = oracle_x0(shape)
    before = model.encode(x.to(DEV))
    x0 = model.encode(x.to(DEV), level="gmlp")
    assert x0.shape == (shape[0], shape[1] // 8, shape[2] // 8, 256) and x0.dtype == torch.float32 and not x0.requires_grad
    rel = float((x0.double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print(precision, shape, f"rel {rel:.2e}")
    assert rel < STAGE_REL, rel
    assert bool((x0 >= 0).all())
    y, r = model.encode(x.to(DEV), level="rcab")
    assert bits_equal(r - x0, y)                                # the same x0 bits as balf_forward_rcab_inputs computes
    assert bits_equal(model.encode(x.to(DEV)), before)          # nothing of the forward's state was changed


def test_encode_gmlp_in_chunks_is_the_concatenation():
    model = synthetic_model(3, "fp32")
    g = torch.Generator().manual_seed(10)
    x = torch.rand((3, 3, 64, 128), generator=g).to(DEV)
    whole = model.encode(x, level="gmlp")
    parts = [model.encode(x[i:i + 1], level="gmlp") for i in range(3)]
    halves = model.encode(x, chunk=2, level="gmlp")
    assert bits_equal(whole, torch.cat(parts)) and bits_equal(halves, whole)
    with pytest.raises(ValueError):
        model.encode(x, level="x1")


def test_train_mixer_tail_end_to_end():
    """The chunk of tests/test_head_train_gpu.py: one pair of 64 x 64 windows with dense labels, presented six times to
    Adam(lr = 1e-3), here through the layer, the block and the head."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    chunk = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(chunk) == 1 and chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = synthetic_model(2, "fp32")
    x = chunk[0][0]
    before = train_utils.check_val_anchor_loss(chunk, model, DEV)
    mixer = TrainableMixerTail.from_model(model)
    assert mixer.encode_level == "gmlp" and sum(p.numel() for p in mixer.gmlp_parameters()) == 668544
    key = model._weights_key(DEV)
    opt = torch.optim.Adam(mixer.parameters(), lr=1e-3)
    gpu = [train_utils.train_head(chunk, model, mixer, opt, DEV, noise=False) for _ in range(6)]
    assert model._weights_key(DEV) == key                       # the model was not touched: no re-pack while training
    assert int(mixer.tail.head.norm.num_batches_tracked) == 12
    # the same six presentations in float64 on the CPU, from the same features
    feats = [(model.encode(b[0], level="gmlp").cpu(), model.encode(b[1], level="gmlp").cpu(), b[2].cpu(), b[3].cpu()) for b in chunk]
    sd = synth.synthetic_state_dict(2)
    hp, running = H.params_of(sd)
    cpu = G.train64(feats, G.params_of(sd), R.params_of(sd), hp, running, 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; GPU", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    # the fourth decimal, as tests/test_rcab_train_gpu.py: Adam's update is a continuous function of the gradients, which agree to
    # ~1e-6 of their scales, and the float32 loss itself carries ~1e-7 of a value of a few units
    assert max(abs(a - b) for a, b in zip(gpu, cpu)) <= 5e-5
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    mixer.commit(model)
    assert model._weights_key(DEV) != key
    got, want = model.eval()(x)["logits"], mixer.eval()(model.encode(x, level="gmlp"))["logits"]
    assert float((got - want).abs().max()) <= LOGIT_TOL
    after = train_utils.check_val_anchor_loss(chunk, model, DEV)
    print(f"check_val_anchor_loss before {before:.4f} after {after:.4f}")
    assert after < before


def test_argument_errors():
    """Each is a return code of the library; nothing is launched (the outputs keep their NaN)."""
    l = ops.lib()
    shape = (1, 8, 8)
    x0, p, g = G.sweep_case(shape, 70)
    d = [p[k].to(DEV) for k in G.PARAMS]
    xd, gd = x0.to(DEV), g.to(DEV)
    y = torch.full(xd.shape, float("nan"), device=DEV)
    grads = [torch.full(t.shape, float("nan"), device=DEV) for t in d]
    saved = torch.empty(l.balf_gmlp_train_saved_bytes(*shape), dtype=torch.uint8, device=DEV)
    ws = torch.empty(l.balf_gmlp_train_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    arr = lambda ts: (C.c_void_p * len(ts))(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])   # noqa: E731
    P, Gr = arr(d), arr(grads)
    ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -3

    def fwd(x=xd.data_ptr(), params=P, dims=shape, out=y.data_ptr(), sv=saved.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return l.balf_gmlp_train_forward(x, params, *dims, out, sv, w, wb, None)

    def bwd(dy=gd.data_ptr(), x=xd.data_ptr(), params=P, sv=saved.data_ptr(), dims=shape, gr=Gr, dx0=None, w=ws.data_ptr(),
            wb=ws.numel()):
        return l.balf_gmlp_train_backward(dy, x, params, sv, *dims, gr, dx0, w, wb, None)

    assert l.balf_error_string(ERR_SHAPE) and l.balf_error_string(ERR_WORKSPACE)
    for dims in ((1, 12, 8), (1, 8, 12)):                       # Hc or Wc no multiple of 8
        assert fwd(dims=dims) == ERR_SHAPE and bwd(dims=dims) == ERR_SHAPE
        assert l.balf_gmlp_train_workspace_bytes(*dims) == 0 and l.balf_gmlp_train_saved_bytes(*dims) == 0
    assert fwd(dims=(0, 8, 8)) == ERR_ARG and fwd(dims=(65536, 8, 8)) == ERR_ARG and l.balf_gmlp_train_saved_bytes(0, 8, 8) == 0
    assert fwd(dims=(4097, 64, 64)) == ERR_SHAPE                # N > 2^24
    assert fwd(x=None) == ERR_ARG and fwd(out=None) == ERR_ARG and fwd(sv=None) == ERR_ARG and fwd(w=None) == ERR_ARG
    assert fwd(params=None) == ERR_ARG and bwd(gr=None) == ERR_ARG and bwd(dy=None) == ERR_ARG and bwd(sv=None) == ERR_ARG
    hole = [t.data_ptr() for t in d]
    hole[17] = None
    assert fwd(params=arr(hole)) == ERR_ARG and bwd(params=arr(hole)) == ERR_ARG and bwd(gr=arr(hole)) == ERR_ARG
    assert fwd(x=xd.data_ptr() + 4) == ERR_ARG and fwd(out=y.data_ptr() + 8) == ERR_ARG and fwd(sv=saved.data_ptr() + 4) == ERR_ARG
    assert bwd(dy=gd.data_ptr() + 4) == ERR_ARG and bwd(dx0=y.data_ptr() + 4) == ERR_ARG and bwd(w=ws.data_ptr() + 8) == ERR_ARG
    assert fwd(wb=ws.numel() - 1) == ERR_WORKSPACE and bwd(wb=ws.numel() - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and all(bool(torch.isnan(t).all()) for t in grads)
    assert fwd() == 0 and bwd() == 0                            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(t).all()) for t in grads)
    # the wrappers refuse from the metadata
    with pytest.raises(ops.BalfHipError):
        ops.gmlp_train_forward(torch.zeros((1, 12, 8, 256), device=DEV), d)
