"""The parts of the stage-4 training path that need no GPU: the fixture linrelu_train.npz and its gates, the float64 restatement
against float64 autograd, what the ``edges`` case must show, the argument checks of the C ABI and of the Python wrappers, and
TrainableStage4's state handling."""
import ctypes as C
import os

import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.model import get_model
from balf_amd.model.stage4_train import TrainableStage4
from balf_amd.utils import synth
from tests import gmlp_train_common as G
from tests import linrelu_train_common as L


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return L.fixture()


@pytest.fixture(scope="module")
def cases(fx):
    """name -> (inputs, restate64 of them), computed once."""
    out = {}
    for name in L.FIXTURE_CASES:
        c = L.fixture_case(fx, name)
        out[name] = (c, L.restate64(*c))
    return out


def test_fixture_digest_and_gates(fx):
    assert list(fx["meta.names"]) == list(L.FIXTURE_CASES)
    assert os.path.getsize(L.FIXTURE) < 1000000
    for name in L.FIXTURE_CASES:
        assert str(fx[f"{name}.inputs_sha256"]) == L.regenerated_inputs_digest(name), name
    for k in L.GATED:
        d, tol = float(fx[f"d_{k}"]), float(fx[f"tol_{k}"])
        assert tol == max(4 * d, L.TOL_FLOOR) and 0 < d < 1e-6, (k, d, tol)
    assert fx["model.x"].shape == (2, 8, 8, 128) and fx["model.g"].shape == (2, 8, 8, 256) and fx["model.dlogits"].shape == (2, 65, 8, 8)
    assert fx["model.y"].shape == (2, 8, 8, 256) and bool((fx["model.y"] >= 0).all())
    assert fx["c32.y"].shape == (70, 64) and fx["c64.dw"].shape == (128, 64) and fx["edges.dx"].shape == (L.EDGES_N, 128)


def test_params_match_the_model():
    assert tuple(L.PARAMS) == tuple(ops.LINRELU_PARAMS)
    sd = get_model.load_model(arch.DEFAULT_MODEL_CFG).state_dict()
    assert tuple(sd[L.SD_PREFIX + "weight"].shape) == (256, 128) and tuple(sd[L.SD_PREFIX + "bias"].shape) == (256,)
    for c_in, stage in ((32, 2), (64, 3), (128, 4)):            # the same layer opens stages 2 and 3
        assert tuple(sd[f"down{stage}.conv.0.weight"].shape) == (2 * c_in, c_in)


@pytest.mark.parametrize("name", L.FIXTURE_CASES)
def test_restatement_against_autograd_and_the_recorded_reference(fx, cases, name):
    (x, w, b, g), res = cases[name]
    ag = L.autograd64(x, w, b, g)
    for k in L.GRADS:
        assert L.err(ag[k], res[k], res["S"][k]) <= 1e-12, k
    y64 = torch.relu(torch.nn.functional.linear(x.double(), w.double(), b.double()))
    assert L.err(y64, res["y"], res["S"]["y"]) == 0.0
    for k in L.GATED:                                           # the reference's own float32 results, as recorded
        e = L.err(torch.from_numpy(fx[f"{name}.{k}"]), res[k], res["S"][k])
        assert e <= float(fx[f"d_{k}"]) * (1 + 1e-6) + 1e-15 <= float(fx[f"tol_{k}"]), (k, e)
    # the distance from the kink, against the float32 movement of y that the recorder measured on the reference's result
    assert L.kink_distance(res) == float(fx[f"{name}.kink"]) > L.KINK_FACTOR * float(fx[f"{name}.moved"])
    assert bool(((torch.from_numpy(fx[f"{name}.y"]).reshape(res["h"].shape) > 0) == (res["h"] > 0)).all())
    # the float32 torch-op composition states the same function
    y, g32 = L.compose_f32(x, w, b, g)
    assert L.err(y, res["y"], res["S"]["y"]) <= float(fx["tol_y"])
    for k in L.GRADS:
        assert L.err(g32[k], res[k], res["S"][k]) <= float(fx[f"tol_{k}"]), k


def test_restatement_edges(cases):
    """What the ``edges`` case must show."""
    (x, w, b, g), res = cases["edges"]
    h, gm = res["h"], res["gm"]
    at = L.EDGES_ZERO_ROW
    assert bool((x[at] == 0).all()) and bool((h[at, :8] == 0).all()) and bool((g[at, :8] != 0).all())
    assert bool((gm[at, :8] == 0).all())                        # the derivative at exactly 0 is 0
    assert float(res["dx"][at].abs().max()) > 0                 # the zero row still receives a gradient
    for c in (L.EDGES_DEAD, 200):                               # dead on every pixel under a huge g: exact zeros, not 0 * 1e30 sums
        assert bool((h[:, c] < 0).all()) and bool((g[:, c].abs() == L.EDGES_HUGE).all())
        assert float(res["db"][c]) == 0.0 and bool((res["dw"][c] == 0).all())
    assert bool((w[L.EDGES_DEAD] == 0).all()) and float(w[200].abs().max()) > 0
    for c, v in L.EDGES_BIAS:
        assert float(b[c]) == v and bool(((h[:, c] > 0) == (v > 0)).all())
    assert all(torch.isfinite(res[k]).all() for k in L.GRADS) and res["S"]["db"] < 100
    # a mask made by multiplying would agree here (0 * 1e30 = 0); one that took h >= 0 would not
    wrong = torch.where(h >= 0, g.double(), torch.zeros_like(h)).sum(0)
    assert float((wrong - res["db"]).abs().max()) >= 1.0


def test_sweep_inputs_are_exact():
    """Every pre-activation of the sweep is an odd multiple of 1/256, exact in float32."""
    for n, c_in in ((64, 32), (257, 64), (63, 128)):
        x, w, b, g = L.sweep_case(n, c_in, 1)
        res = L.restate64(x, w, b, g)
        h = res["h"] * 256
        assert bool((h == h.round()).all()) and bool((h.round().long() % 2 == 1).all()) and L.kink_distance(res) >= 1 / 256
        assert bool((torch.nn.functional.linear(x, w, b).double() == res["h"]).all())
        assert 0.3 < float((res["h"] > 0).double().mean()) < 0.7 and float((g == 0).float().mean()) > 0.03


def test_abi_symbols_and_argument_checks(lib):
    for name in ("balf_linrelu_train_workspace_bytes", "balf_linrelu_train_forward", "balf_linrelu_train_backward"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    fake = C.c_void_p(4096)
    n, c_in = 100, 128
    ws = lib.balf_linrelu_train_workspace_bytes(n, c_in)
    assert ws >= n * 256 * 4 + 256 * 128 * 4

    def fwd(dims=(n, c_in), x=fake, w=fake, b=fake, y=fake):
        return lib.balf_linrelu_train_forward(x, w, b, *dims, y, None)

    def bwd(dims=(n, c_in), nbytes=ws, g=fake, y=fake, x=fake, w=fake, dw=fake, db=fake, dx=None, work=fake):
        return lib.balf_linrelu_train_backward(g, y, x, w, *dims, dw, db, dx, work, nbytes, None)

    for k in ("x", "w", "b", "y"):
        assert fwd(**{k: None}) == -1 and fwd(**{k: C.c_void_p(4100)}) == -1, k
    for k in ("g", "y", "x", "w", "dw", "db", "work"):
        assert bwd(**{k: None}) == -1 and bwd(**{k: C.c_void_p(4104)}) == -1, k
    assert bwd(dx=C.c_void_p(4100)) == -1
    for call in (fwd, bwd):
        for bad in (0, 16, 48, 96, 256, -32):
            assert call(dims=(n, bad)) == -1, bad
        assert call(dims=(0, c_in)) == -2 and call(dims=(-5, c_in)) == -2 and call(dims=((1 << 24) + 1, 32)) == -2
    assert bwd(nbytes=ws - 1) == -3 and bwd(dims=(n + 1000, c_in)) == -3
    assert [lib.balf_linrelu_train_workspace_bytes(*bad) for bad in ((0, 128), (1, 16), (1, 256), ((1 << 24) + 1, 64), (-1, 32))] == [0] * 5
    for c in L.WIDTHS:
        sizes = [lib.balf_linrelu_train_workspace_bytes(v, c) for v in (1, 63, 64, 257, 960, 17408, 1 << 20, 1 << 24)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] >= (1 << 24) * 2 * c * 4


def test_python_layers_refuse_before_touching_a_device():
    x, w, b, g = L.sweep_case(64, 128, 1)
    y = torch.zeros(64, 256)
    with pytest.raises(_lib.BalfHipError, match="GPU"):                      # CPU tensors
        ops.linrelu_train_forward(x, w, b)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.linrelu_train_backward(g, y, x, w)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.linrelu_train_forward(x.reshape(2, 4, 8, 128), w, b)
    for bad in (torch.zeros(4, 48), torch.zeros(4, 256), torch.zeros(128), torch.zeros(0, 128)):
        with pytest.raises(_lib.BalfHipError, match="c_in one of|2\\^24"):
            ops.linrelu_train_forward(bad, w, b)
    with pytest.raises(_lib.BalfHipError, match="x must be float32"):
        ops.linrelu_train_forward(x.double(), w, b)
    with pytest.raises(_lib.BalfHipError, match="weight must be float32"):
        ops.linrelu_train_forward(x, w.half(), b)
    with pytest.raises(_lib.BalfHipError, match="weight must be \\[256, 128\\]"):
        ops.linrelu_train_forward(x, w.T.contiguous(), b)
    with pytest.raises(_lib.BalfHipError, match="weight must be \\[128, 64\\]"):
        ops.linrelu_train_forward(x[:, :64].contiguous(), w, b)
    with pytest.raises(_lib.BalfHipError, match="bias must be"):
        ops.linrelu_train_forward(x, w, b[:128])
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.linrelu_train_forward(x, w.T.contiguous().T, b)
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.linrelu_train_forward(torch.zeros(128, 64).T, w, b)
    with pytest.raises(_lib.BalfHipError, match="16-byte"):                  # a view one float into its storage
        ops.linrelu_train_forward(torch.zeros(x.numel() + 1)[1:].view(x.shape), w, b)
    with pytest.raises(_lib.BalfHipError, match="g must be"):
        ops.linrelu_train_backward(g[:, :128].contiguous(), y, x, w)
    with pytest.raises(_lib.BalfHipError, match="y must be"):
        ops.linrelu_train_backward(g, y[:32].contiguous(), x, w)
    with pytest.raises(_lib.BalfHipError, match="g must be float32"):
        ops.linrelu_train_backward(g.half(), y, x, w)
    with pytest.raises(_lib.BalfHipError, match="dx must be"):
        ops.linrelu_train_backward(g, y, x, w, want_dx=torch.zeros(64, 256))
    stage = TrainableStage4()
    x3 = torch.zeros(1, 8, 8, 128)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        stage(x3)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        stage.eval()(x3)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    with pytest.raises(_lib.BalfHipError, match="CPU"):
        model.encode(torch.zeros(1, 3, 64, 64), level="stage3")
    with pytest.raises(ValueError, match="'stage3'"):                        # the unknown-level error lists the new level
        model.encode(_FakeCuda(), level="x1")


class _FakeCuda:
    """What encode looks at before the level: a [1,3,64,64] input that says it lives on a GPU."""
    shape = (1, 3, 64, 64)
    is_cuda = True

    def dim(self):
        return 4


def test_trainable_stage4_state():
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    sd = synth.synthetic_state_dict(2)
    model.load_state_dict(sd)
    stage = TrainableStage4.from_model(model)
    assert stage.training and stage.mixer.training and stage.mixer.tail.head.training and stage.encode_level == "stage3"
    state = stage.state_dict()
    assert list(state)[:2] == ["conv0.weight", "conv0.bias"]
    assert list(state)[2:] == ["mixer." + k for k in stage.mixer.state_dict()]
    params = list(stage.parameters())
    assert len(params) == 44 and sum(q.numel() for q in params) == sum(q.numel() for q in stage.mixer.parameters()) + 33024
    assert sum(q.numel() for q in stage.conv0_parameters()) == 33024 and sum(q.numel() for q in params) == 949379
    for k, mine in zip(ops.LINRELU_PARAMS, stage.conv0_parameters()):
        assert torch.equal(mine, sd[L.SD_PREFIX + k]) and mine.data_ptr() != model.state_dict()[L.SD_PREFIX + k].data_ptr(), k
    key = model._weights_key("cpu")
    with torch.no_grad():                                                # what an optimiser step does to the copies
        for q in stage.parameters():
            q.add_(1.0)
    assert model._weights_key("cpu") == key
    assert torch.equal(model.state_dict()[L.SD_PREFIX + "weight"], sd[L.SD_PREFIX + "weight"])
    stage.commit(model)
    assert model._weights_key("cpu") != key
    after = model.state_dict()
    for k in ops.LINRELU_PARAMS:
        assert torch.equal(after[L.SD_PREFIX + k], sd[L.SD_PREFIX + k] + 1.0), k
    for k in (G.SD_PREFIX + "dense1.weight", "down4.residual_channel_attention_block.conv1.weight", "down4.conv2.weight",
              "detector_head.dense.bias"):
        assert torch.equal(after[k], sd[k] + 1.0), k
    for k in ("down3.conv.0.weight", "down3.conv.0.bias"):
        assert torch.equal(after[k], sd[k]), k                           # stage 3 stays frozen
    stage.eval()
    assert not stage.mixer.training and not stage.mixer.tail.head.training
