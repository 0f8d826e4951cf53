"""The training-mode head without a GPU: the float64 restatement against the reference's recorded results
(tests/golden/head_train.npz) and against float64 autograd, the argument checks of the C ABI on fake pointers, the Python
layers' refusals before any device is touched, and the state handling of TrainableHead."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.model import get_model
from balf_amd.model.head_train import TrainableHead
from balf_amd.utils import synth, train_utils
from tests import head_train_common as H


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return H.fixture()


def test_fixture_holds_the_cases_and_the_gates(fx):
    assert tuple(str(n) for n in fx["meta.names"]) == H.FIXTURE_CASES
    assert fx["model.x2"].shape == (2, 8, 8, 256) and fx["model.x2"].dtype == np.float32
    for name, (b, hc, wc) in (("model", (2, 8, 8)), ("edges", H.EDGES_SHAPE)):
        assert fx[f"{name}.logits"].shape == (b, 65, hc, wc) and fx[f"{name}.dx2"].shape == (b, hc, wc, 256)
        assert fx[f"{name}.dw2"].shape == (256, 256) and fx[f"{name}.dw2"].dtype == np.float32
        assert fx[f"{name}.dwd"].shape == (65, 256) and fx[f"{name}.db2"].shape == (256,)
        for k in ("dbd", "dgamma", "dbeta", "running_mean", "running_var"):
            assert fx[f"{name}.{k}"].shape == (65,)
        assert float(fx[f"{name}.kink"]) >= H.KINK_MARGIN
        # the inputs that are regenerated rather than stored are still the ones the reference's results were recorded on
        assert str(fx[f"{name}.inputs_sha256"]) == H.regenerated_inputs_digest(name), name
    for k in H.GATED:
        assert float(fx[f"tol_{k}"]) == max(4 * float(fx[f"d_{k}"]), H.TOL_FLOOR)
        assert 0 < float(fx[f"d_{k}"]) < 1e-6 and float(fx[f"tol_{k}"]) < 5e-6
    assert os.path.getsize(H.FIXTURE) < 1 << 20


@pytest.mark.parametrize("name", H.FIXTURE_CASES)
def test_restatement_reproduces_the_reference(fx, name):
    x2, p, dlogits, running = H.fixture_case(fx, name)
    r = H.restate64(x2, p, dlogits, running=running)
    for k in H.GATED:
        e = H.err(fx[f"{name}.{k}"], r[k], r["S"][k])
        assert e <= float(fx[f"d_{k}"]) * (1 + 1e-9) <= float(fx[f"tol_{k}"]), (k, e)
    ag = H.autograd64(x2, p, dlogits)
    for k in H.GRADS:
        assert H.err(ag[k], r[k], r["S"][k]) <= 1e-12, k
    assert H.kink_distance(r["h"]) == float(fx[f"{name}.kink"])
    # the float32 torch-op composition (what tools/bench_head_train.py times) states the same function
    logits32, g32 = H.compose_f32(x2, p, dlogits, running=(running[0].clone(), running[1].clone()))
    assert H.err(logits32, r["logits"], r["S"]["logits"]) <= float(fx["tol_logits"])
    for k in H.GRADS:
        assert H.err(g32[k], r[k], r["S"][k]) <= float(fx[f"tol_{k}"]), k


def test_restatement_edges():
    """What the ``edges`` case must show: exact zeros at the kink with a zero derivative, a channel whose gamma is 0 and whose
    dgamma is not, a channel whose mean^2 dwarfs its variance, dbd analytically zero."""
    x2, p, dlogits, running = H.edges_inputs()
    r = H.restate64(x2, p, dlogits, running=running)
    h, dh = r["h"].reshape(*H.EDGES_SHAPE, 256), r["dh"].reshape(*H.EDGES_SHAPE, 256)
    for at in H.EDGES_ZERO_ROWS:
        assert bool((h[at][:8] == 0).all()) and bool((dh[at][:8] == 0).all()) and bool((h[at][8:] != 0).all())
    c = H.EDGES_GAMMA0
    assert float(p["gamma"][c]) == 0 and float(r["dgamma"][c].abs()) > 1e-3 * r["S"]["dgamma"]
    assert bool((r["dz"][:, c] == 0).all()) and bool((r["logits"][:, c] == p["beta"][c].double()).all())
    c = H.EDGES_SHIFTED
    assert float(r["mean"][c] ** 2 / r["var"][c]) > 1e3
    assert float(r["dbd"].abs().max()) < 1e-12 * r["S"]["dbd"]
    # eval mode: the supplied statistics, no running update
    e = H.restate64(x2, p, stats=torch.stack(running), running=running)
    assert "running_mean" not in e and not torch.equal(e["logits"], r["logits"])


def test_sweep_cases_stay_off_the_kink():
    x2, p, _, _ = H.sweep_case((2, 7, 9), 3)
    X = x2.reshape(-1, 256)
    h32 = X @ p["w2"].T + p["b2"]
    h64 = X.double() @ p["w2"].double().T + p["b2"].double()
    assert torch.equal(h32.double(), h64) and float(h64.abs().min()) >= 1 / 256       # exact in float32, never at the kink
    assert 0.2 < float((h64 > 0).double().mean()) < 0.8
    for shape in ((1, 1, 2), (2, 1, 1)):                        # N = 2: z is exact as well, and no channel is constant
        x2, p, dlogits, running = H.sweep_case(shape, 7 + shape[1] * 100 + shape[2])
        r = H.restate64(x2, p, dlogits, running=running)
        z32 = r["a"].float() @ p["wd"].T + p["bd"]
        assert torch.equal(r["a"].float().double(), r["a"]) and torch.equal(z32.double(), r["z"])
        assert float(r["var"].min()) > 0


def test_abi_argument_checks(lib):
    fake = C.c_void_p(4096)
    n = 2 * 3 * 5
    ws, sv = lib.balf_head_train_workspace_bytes(n), lib.balf_head_train_saved_bytes(n)
    assert ws > 0 and sv >= n * (256 + 65) * 4 + 2 * 65 * 8

    def fwd(b=2, hc=3, wc=5, nbytes=ws, use_stats=0, **kw):
        a = dict(x2=fake, w2=fake, b2=fake, wd=fake, bd=fake, gamma=fake, beta=fake, stats=None, logits=fake, saved=fake, work=fake)
        a.update(kw)
        return lib.balf_head_train_forward(a["x2"], a["w2"], a["b2"], a["wd"], a["bd"], a["gamma"], a["beta"], b, hc, wc, 1e-5,
                                           use_stats, a["stats"], a["logits"], None, None, None, 0.1, a["saved"], a["work"],
                                           nbytes, None)

    def bwd(b=2, hc=3, wc=5, nbytes=ws, **kw):
        a = dict(g=fake, x2=fake, w2=fake, wd=fake, gamma=fake, saved=fake, dw2=fake, db2=fake, dwd=fake, dbd=fake, dgamma=fake,
                 dbeta=fake, work=fake)
        a.update(kw)
        return lib.balf_head_train_backward(a["g"], a["x2"], a["w2"], a["wd"], a["gamma"], a["saved"], b, hc, wc, a["dw2"],
                                            a["db2"], a["dwd"], a["dbd"], a["dgamma"], a["dbeta"], None, a["work"], nbytes, None)

    for k in ("x2", "w2", "b2", "wd", "bd", "gamma", "beta", "logits", "saved", "work"):
        assert fwd(**{k: None}) == -1, k
    for k in ("g", "x2", "w2", "wd", "gamma", "saved", "dw2", "db2", "dwd", "dbd", "dgamma", "dbeta", "work"):
        assert bwd(**{k: None}) == -1, k
    assert fwd(use_stats=1) == -1                                   # use_stats without statistics
    for call in (fwd, bwd):
        assert call(b=1, hc=1, wc=1) == -1                          # N = 1: no variance
        assert call(b=0) == -1 and call(b=65536) == -1 and call(hc=0) == -1 and call(wc=-1) == -1
        assert call(b=1, hc=4096, wc=4097, nbytes=1 << 60) == -2    # N > 2^24
        assert call(b=3, hc=2048, wc=4096, nbytes=1 << 60) == -2
        assert call(work=C.c_void_p(4100)) == -1 and call(saved=C.c_void_p(4100)) == -1      # float64 lives in both
        assert call(nbytes=ws - 1) == -3
    for query in (lib.balf_head_train_workspace_bytes, lib.balf_head_train_saved_bytes):
        assert [query(bad) for bad in (-5, 0, 1, (1 << 24) + 1)] == [0, 0, 0, 0]
        sizes = [query(v) for v in (2, 64, 65, 256, 257, 1702, 4096, 81920, 1 << 20, 1 << 24)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]


def test_python_layers_refuse_before_touching_a_device():
    x2, p, dlogits, running = H.sweep_case((2, 3, 5), 1)
    args = dict(x2=x2, **p)
    with pytest.raises(_lib.BalfHipError, match="GPU"):                      # CPU tensors
        ops.head_train_forward(**args)
    saved = torch.zeros(1 << 20, dtype=torch.uint8)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.head_train_backward(dlogits, x2, p["w2"], p["wd"], p["gamma"], saved)
    for k in ("x2", "w2", "b2", "wd", "bd", "gamma", "beta"):
        with pytest.raises(_lib.BalfHipError, match="float32"):              # wrong dtypes
            ops.head_train_forward(**{**args, k: args[k].double()})
    with pytest.raises(_lib.BalfHipError, match="float32"):
        ops.head_train_forward(**args, stats=torch.stack(running).double())
    with pytest.raises(_lib.BalfHipError, match="float32"):
        ops.head_train_backward(dlogits.half(), x2, p["w2"], p["wd"], p["gamma"], saved)
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.head_train_forward(**{**args, "x2": x2.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)})
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.head_train_forward(**{**args, "w2": p["w2"].T})
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.head_train_backward(dlogits.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), x2, p["w2"], p["wd"], p["gamma"], saved)
    with pytest.raises(_lib.BalfHipError, match="256"):                      # wrong channel counts
        ops.head_train_forward(**{**args, "x2": x2[..., :128].contiguous()})
    with pytest.raises(_lib.BalfHipError, match="wd must be"):
        ops.head_train_forward(**{**args, "wd": p["wd"][:64].contiguous()})
    with pytest.raises(_lib.BalfHipError, match="gamma must be"):
        ops.head_train_forward(**{**args, "gamma": p["gamma"][:64].contiguous()})
    with pytest.raises(_lib.BalfHipError, match="dlogits must be"):
        ops.head_train_backward(dlogits[:, :64].contiguous(), x2, p["w2"], p["wd"], p["gamma"], saved)
    with pytest.raises(_lib.BalfHipError, match="2 <= B"):                   # one pixel has no variance
        ops.head_train_forward(**{**args, "x2": x2[:1, :1, :1].contiguous()})
    head = TrainableHead()
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        head(x2)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        head.eval()(x2)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    with pytest.raises(_lib.BalfHipError, match="CPU"):
        model.encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        model.encode(torch.zeros(1, 1, 64, 64))


def test_trainable_head_state():
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    sd = synth.synthetic_state_dict(2)
    model.load_state_dict(sd)
    head = TrainableHead.from_model(model)
    assert head.training
    state = head.state_dict()
    assert list(state) == ["conv2.weight", "conv2.bias", "dense.weight", "dense.bias", "norm.weight", "norm.bias",
                           "norm.running_mean", "norm.running_var", "norm.num_batches_tracked"]
    assert [n for n, _ in head.named_parameters()] == list(state)[:6]
    assert torch.equal(state["conv2.weight"], sd["down4.conv2.weight"]) and torch.equal(state["norm.running_var"],
                                                                                        sd["detector_head.norm.running_var"])
    assert state["conv2.weight"].data_ptr() != model.down4.conv2.weight.data_ptr()           # copies
    key = model._weights_key("cpu")
    with torch.no_grad():                                                # what an optimiser step and a forward do to the copies
        for q in head.parameters():
            q.add_(1.0)
        head.norm.running_mean.mul_(0.5)
        head.norm.num_batches_tracked += 3
    assert model._weights_key("cpu") == key
    assert torch.equal(model.down4.conv2.weight, sd["down4.conv2.weight"])
    head.commit(model)
    assert model._weights_key("cpu") != key
    after = model.state_dict()
    for mine, theirs in (("conv2.weight", "down4.conv2.weight"), ("conv2.bias", "down4.conv2.bias"),
                         ("dense.weight", "detector_head.dense.weight"), ("dense.bias", "detector_head.dense.bias"),
                         ("norm.weight", "detector_head.norm.weight"), ("norm.bias", "detector_head.norm.bias"),
                         ("norm.running_mean", "detector_head.norm.running_mean"),
                         ("norm.running_var", "detector_head.norm.running_var")):
        assert torch.equal(after[theirs], head.state_dict()[mine]), mine
    assert torch.equal(after["down4.conv2.weight"], sd["down4.conv2.weight"] + 1.0)
    assert int(after["detector_head.norm.num_batches_tracked"]) == 3
    assert torch.equal(after["down1.conv.0.weight"], sd["down1.conv.0.weight"])              # the encoder is left alone


def test_train_head_refusals():
    with pytest.raises(ValueError, match="empty"):
        train_utils.train_head([], None, TrainableHead(), None, "cpu")
    with pytest.raises(ValueError, match="grid_size=8"):
        train_utils.train_head([], None, TrainableHead(), None, "cpu", grid_size=16)


class _StubModel:
    """The guard's faces that train_head sees, with a scripted course: ``flag_at`` = which encode (counted from 0) is the
    flagged split-f16 forward; ``consumed_in_flight``: a later forward's own look finds that flag (verdict set, nothing for the
    final check to find) instead of the final check."""

    def __init__(self, flag_at=None, consumed_in_flight=False, precision="fp16"):
        self.effective_precision = precision
        self.flag_at, self.consumed_in_flight = flag_at, consumed_in_flight
        self.encodes, self.pending_flag, self.checks = [], False, 0

    def encode(self, x):
        if self.pending_flag and self.consumed_in_flight:       # this forward's lazy look at the earlier one
            self.pending_flag, self.effective_precision = False, "fp32"
        flagged = self.effective_precision == "fp16" and len(self.encodes) == self.flag_at
        self.pending_flag = self.pending_flag or flagged
        self.encodes.append((x, self.effective_precision, flagged))
        return (x, self.effective_precision, flagged)

    def fp16_guard_check(self, synchronize=True):
        assert synchronize
        self.checks += 1
        if self.pending_flag:
            self.pending_flag, self.effective_precision = False, "fp32"
            return True
        return False


@pytest.mark.parametrize("flag_at,in_flight,precision,encodes", [
    (None, False, "fp16", 4),       # no flag: the chunk is encoded once
    (3, False, "fp16", 8),          # the last forward is flagged: the final check finds it
    (0, True, "fp16", 8),           # the first is flagged and a later forward of the chunk consumes the flag: the check says False
    (0, False, "fp16", 8),
    (None, False, "fp32", 4),       # already on the fp32 kernels: nothing to repeat
])
def test_train_head_encodes_again_when_the_flag_was_consumed_in_flight(flag_at, in_flight, precision, encodes):
    model = _StubModel(flag_at, in_flight, precision)
    batches = [("s0", "d0"), ("s1", "d1")]
    feats = train_utils._guarded_features(model, lambda: [(model.encode(b[0]), model.encode(b[1])) for b in batches])
    assert len(model.encodes) == encodes and model.checks == 1
    assert [(f[0][0], f[1][0]) for f in feats] == batches
    assert not any(f[side][2] for f in feats for side in (0, 1))           # no flagged forward's features are returned
    if flag_at is not None:
        assert all(f[side][1] == "fp32" for f in feats for side in (0, 1))
