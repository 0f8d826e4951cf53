"""detector_loss without a GPU: the float64 restatement against the reference's recorded loss and gradient
(tests/golden/detector_loss.npz), the argument checks of the C ABI, and the Python layers' refusals, all before any device
is touched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd.loss import loss_function
from balf_amd.utils import train_utils
from tests import detector_loss_common as D


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return D.fixture()


def fixture_case(fx, name):
    t = {k: torch.from_numpy(fx[f"{name}.{k}"].astype(np.float32)) for k in ("logits", "keypoint_map", "noise")}
    t["valid_mask"] = torch.from_numpy(fx[f"{name}.valid_mask"].astype(np.float32)) if f"{name}.valid_mask" in fx else None
    return t


def test_fixture_holds_the_cases_and_the_gates(fx):
    assert [str(n) for n in fx["meta.names"]] == [c[0] for c in D.FIXTURE_CASES]
    for name, shape, _, _, with_mask in D.FIXTURE_CASES:
        b, hc, wc = shape
        assert fx[f"{name}.logits"].shape == (b, 65, hc, wc) and fx[f"{name}.keypoint_map"].shape == (b, 1, 8 * hc, 8 * wc)
        assert (f"{name}.valid_mask" in fx) == with_mask
    assert float(fx["tol_loss"]) == max(4 * float(fx["d_loss"]), D.TOL_FLOOR)
    assert float(fx["tol_grad"]) == max(4 * float(fx["d_grad"]), D.TOL_FLOOR)
    assert float(fx["tol_loss"]) < 1e-5 and float(fx["tol_grad"]) < 1e-5
    assert os.path.getsize(D.FIXTURE) < 1 << 20


@pytest.mark.parametrize("name", [c[0] for c in D.FIXTURE_CASES])
def test_restatement_reproduces_the_reference(fx, name):
    c = fixture_case(fx, name)
    r = D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"])
    assert np.array_equal(r["labels"], fx[f"{name}.labels"])
    # float64 against the recorded float64: the same statements, but a CPU's vector width decides the order inside torch's sums
    # and the last bit of its exp, so equal to a few float64 roundings (2.2e-16 each, sums of at most 135 terms), not bit for bit
    assert D.loss_error(r["loss"], fx[f"{name}.loss64"]) <= 1e-12 and D.loss_error(r["per_image"], fx[f"{name}.per_image64"]) <= 1e-12
    assert D.grad_error(r["grad"], fx[f"{name}.grad64"], fx[f"{name}.den64"]) <= 1e-12
    assert D.loss_error(fx[f"{name}.loss"], r["loss"]) <= float(fx["tol_loss"])
    assert D.grad_error(fx[f"{name}.grad"], r["grad"], r["den"]) <= float(fx["tol_grad"])
    # the float32 torch-op composition (what tools/bench_loss.py times) states the same loss
    loss32, grad32 = D.compose_f32(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"], want_grad=True)
    assert D.loss_error(loss32.numpy(), r["loss"]) <= float(fx["tol_loss"])
    assert D.grad_error(grad32.numpy(), r["grad"], r["den"]) <= float(fx["tol_grad"])


def test_restatement_edges():
    """What the fixture must show: a fully masked image gives 0, the logits x 100 case needs the maximum taken out."""
    c = D.make_case((2, 2, 3), 5)
    r = D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], None)
    assert r["per_image"][-1] == 0.0 and not r["grad"][-1].any() and r["per_image"][0] > 0
    kp = torch.zeros((1, 1, 8, 16))
    kp[0, 0, 0, 5] = kp[0, 0, 5, 0] = 1.0                       # channels 5 and 40 of cell 0; cell 1 empty
    assert D.labels_f32(kp, None).ravel().tolist() == [5, 64]
    kp[0, 0, 0, 8] = 0.5                                        # 2 * 0.5 ties the dustbin: the lower index wins
    assert D.labels_f32(kp, None).ravel().tolist() == [5, 0]


def test_abi_argument_checks(lib):
    fake = C.c_void_p(4096)
    ws = lib.balf_detector_loss_workspace_bytes(2, 3, 5)
    assert ws > 0

    def call(logits=fake, kp=fake, b=2, hc=3, wc=5, loss=fake, work=fake, nbytes=ws):
        return lib.balf_detector_loss(logits, kp, None, None, b, hc, wc, loss, None, None, None, work, nbytes, None)

    assert call(logits=None) == -1 and call(kp=None) == -1 and call(loss=None) == -1 and call(work=None) == -1
    assert call(b=0) == -1 and call(b=65536) == -1 and call(hc=0) == -1 and call(wc=-1) == -1
    assert call(hc=4096, wc=4097, nbytes=1 << 60) == -2          # Hc * Wc > 2^24
    assert call(work=C.c_void_p(4100)) == -1                     # float64 sums live in the workspace
    assert call(nbytes=ws - 1) == -3
    for bad in ((0, 3, 5), (65536, 3, 5), (1, 0, 5), (1, 4096, 4097)):
        assert lib.balf_detector_loss_workspace_bytes(*bad) == 0
    assert lib.balf_detector_loss_workspace_bytes(1, 4096, 4096) > 0
    sizes = [lib.balf_detector_loss_workspace_bytes(b, hc, wc) for b, hc, wc in ((1, 1, 1), (1, 8, 8), (1, 16, 17), (2, 16, 17),
                                                                                (32, 136, 240), (64, 136, 240))]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]


def test_python_layers_refuse_before_touching_a_device():
    c = D.make_case((2, 3, 5), 1)
    lg, kp, vm, nz = c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"]
    with pytest.raises(_lib.BalfHipError, match="GPU"):                      # CPU tensors
        ops.detector_loss(lg, kp, vm, nz)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        loss_function.detector_loss(kp, lg, vm, noise=False)
    for bad in (dict(logits=lg.double()), dict(keypoint_map=kp.half()), dict(valid_mask=vm.double()), dict(noise=nz.double())):
        with pytest.raises(_lib.BalfHipError, match="float32"):              # wrong dtypes
            ops.detector_loss(**{**dict(logits=lg, keypoint_map=kp, valid_mask=vm, noise=nz), **bad})
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.detector_loss(lg.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), kp, vm, nz)
    with pytest.raises(_lib.BalfHipError, match="65"):
        ops.detector_loss(lg[:, :64].contiguous(), kp)
    with pytest.raises(_lib.BalfHipError, match="keypoint_map must be"):
        ops.detector_loss(lg, kp[:, :, :, :-8].contiguous())
    with pytest.raises(ValueError, match="grid_size=8"):
        loss_function.detector_loss(kp, lg, vm, grid_size=16)
    with pytest.raises(ValueError, match="65"):
        loss_function.detector_loss(kp, lg[:, :64].contiguous())
    with pytest.raises(ValueError, match="H/8"):
        loss_function.detector_loss(kp[:, :, :-8].contiguous(), lg)
    with pytest.raises(ValueError, match="H/8"):
        loss_function.detector_loss(kp[:, :, :, :-4].contiguous(), lg)              # W not a multiple of 8
    with pytest.raises(ValueError, match="device"):
        loss_function.detector_loss(kp, lg, device="cuda")                         # names another device than the tensors'
    with pytest.raises(ValueError, match="empty"):
        train_utils.check_val_anchor_loss([], None, "cpu")
