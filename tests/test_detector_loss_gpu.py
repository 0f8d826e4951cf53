"""balf_detector_loss on the GPU (include/balf_hip.h; ops.detector_loss, loss.loss_function.detector_loss,
utils.train_utils.check_val_anchor_loss) against tests/golden/detector_loss.npz -- the reference's own loss and gradient,
recorded by tests/golden/make_detector_loss_golden.py -- and against the float64 restatement of tests/detector_loss_common.py.
Labels are compared exactly; loss, per-image values and gradient within the fixture's tol_loss / tol_grad
(max(4 * d, 2^-21), d = the reference's own distance from the restatement; normalisations: detector_loss_common.loss_error /
grad_error).  Only the fixture is read here, never the reference tree."""
import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.loss import loss_function
from balf_amd.model import get_model
from balf_amd.utils import synth, train_utils
from tests import detector_loss_common as D
from tests import pair_synth_common as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c[0] for c in D.FIXTURE_CASES]


@pytest.fixture(scope="module")
def fx():
    return D.fixture()


def fixture_case(fx, name):
    t = {k: torch.from_numpy(fx[f"{name}.{k}"].astype(np.float32)) for k in ("logits", "keypoint_map", "noise")}
    t["valid_mask"] = torch.from_numpy(fx[f"{name}.valid_mask"].astype(np.float32)) if f"{name}.valid_mask" in fx else None
    return t


def dev(c):
    return {k: (v.to(DEV) if v is not None else None) for k, v in c.items()}


def run_all(c, **kw):
    d = dev(c)
    return ops.detector_loss(d["logits"], d["keypoint_map"], d["valid_mask"], d["noise"], want_per_image=True, want_labels=True,
                             want_grad=True, **kw)


def check_against(out, r, fx, what):
    assert np.array_equal(out.labels.cpu().numpy(), r["labels"]), what
    e_loss = D.loss_error(out.loss.cpu().numpy(), r["loss"])
    e_img = D.loss_error(out.per_image.cpu().numpy(), r["per_image"])
    e_grad = D.grad_error(out.dlogits.cpu().numpy(), r["grad"], r["den"])
    print(f"{what}: loss err {e_loss:.2e} per-image err {e_img:.2e} (tol {float(fx['tol_loss']):.2e}) grad err {e_grad:.2e} "
          f"(tol {float(fx['tol_grad']):.2e})")
    assert e_loss <= float(fx["tol_loss"]) and e_img <= float(fx["tol_loss"]), what
    assert e_grad <= float(fx["tol_grad"]), what
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.labels.dtype == torch.int32


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity(fx, name):
    c = fixture_case(fx, name)
    out = run_all(c)
    r = {"labels": fx[f"{name}.labels"], "loss": fx[f"{name}.loss64"], "per_image": fx[f"{name}.per_image64"],
         "grad": fx[f"{name}.grad64"], "den": fx[f"{name}.den64"]}
    check_against(out, r, fx, name)
    assert torch.isfinite(out.loss) and torch.isfinite(out.dlogits).all()            # (big_logits: no overflow)
    d = dev(c)
    loss = loss_function.detector_loss(d["keypoint_map"], d["logits"], d["valid_mask"], 8, DEV, noise=d["noise"])
    assert bits_equal(loss, out.loss) and not loss.requires_grad
    # the outputs do not depend on which of them are requested
    only = ops.detector_loss(d["logits"], d["keypoint_map"], d["valid_mask"], d["noise"])
    assert only.per_image is None and only.labels is None and only.dlogits is None and bits_equal(only.loss, out.loss)
    if c["valid_mask"] is None:                                                     # None equals a mask of ones, bit for bit
        ones = run_all({**c, "valid_mask": torch.ones_like(c["keypoint_map"])})
        for a, b in zip(out, ones):
            assert bits_equal(a, b)


# n = Hc * Wc just below, at and above one wave (63, 64, 65), mid-workgroup (135), just below, at and above a 256-lane
# workgroup (255, 256, 257), one-pixel-thin planes
SWEEP = ((1, 1), (7, 9), (8, 8), (5, 13), (9, 15), (15, 17), (16, 16), (1, 257), (257, 1))


@pytest.mark.parametrize("hc,wc", SWEEP)
def test_shape_sweep(fx, hc, wc):
    c = D.make_case((3, hc, wc), 100 + hc * 1000 + wc)
    r = D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"])
    check_against(run_all(c), r, fx, f"{hc}x{wc}")
    c = D.make_case((3, hc, wc), 200 + hc * 1000 + wc, with_mask=False)
    r = D.restate64(c["logits"], c["keypoint_map"], None, None)
    check_against(run_all({**c, "noise": None}), r, fx, f"{hc}x{wc} no mask, no noise")


@pytest.mark.parametrize("b", (16, 17, 37))
def test_more_images_than_one_finish_pass(fx, b):
    """loss_finish_kernel takes sixteen images per pass (a wave each) and loss_sum_kernel four per workgroup: a full pass, one
    image into the second, and a third pass with a ragged tail; the serial mean over B follows."""
    c = D.make_case((b, 2, 3), 500 + b, last_masked=False)
    check_against(run_all(c), D.restate64(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"]), fx, f"B = {b}")


def test_ties_and_edges_without_noise(fx):
    hc, wc = 2, 3
    kp = torch.zeros((1, 1, 8 * hc, 8 * wc))
    kp[0, 0, 0, 5] = kp[0, 0, 5, 0] = 1.0          # cell 0: channels 5 and 40 -> 5
    kp[0, 0, 1, 8 + 2] = 0.5                       # cell 1: 2 * 0.5 ties the dustbin at channel 10 -> the lower index
    kp[0, 0, 8 + 7, 16 + 7] = 1.0                  # cell 5: channel 63
    vm = torch.ones_like(kp)
    vm[0, 0, 8 + 3, 4] = 0.0                       # one zero pixel in cell 3
    c = {"logits": D.make_case((1, hc, wc), 3)["logits"], "keypoint_map": kp, "valid_mask": vm, "noise": None}
    out = run_all(c)
    assert out.labels.cpu().ravel().tolist() == [5, 10, 64, 64, 64, 63]
    g = out.dlogits.cpu()
    assert not g[0, :, 1, 0].any() and g[0, :, 0, 0].any() and g[0, :, 1, 1].any()     # cell 3 exactly zero, its neighbours not
    check_against(out, D.restate64(c["logits"], kp, vm, None), fx, "ties")
    # a fully masked batch: loss 0 and an all-zero gradient
    c = D.make_case((2, 3, 5), 4)
    out = run_all({**c, "valid_mask": torch.zeros_like(c["keypoint_map"])})
    assert float(out.loss) == 0.0 and not out.per_image.any() and not out.dlogits.any()


def test_batch_invariance_and_determinism():
    c = D.make_case((3, 15, 17), 21, last_masked=False)

    def sub(ix):
        return {k: (v[ix].contiguous() if v is not None else None) for k, v in c.items()}

    abc, abc2 = run_all(c), run_all(c)
    for a, b in zip(abc, abc2):
        assert bits_equal(a, b)
    only_c, ca = run_all(sub([2])), run_all(sub([2, 0]))
    assert bits_equal(only_c.per_image[0], abc.per_image[2]) and bits_equal(ca.per_image[0], abc.per_image[2])
    assert bits_equal(ca.per_image[1], abc.per_image[0])
    assert torch.equal(only_c.labels[0], abc.labels[2]) and float(abc.per_image[2]) > 0


def test_autograd(fx, monkeypatch):
    name = "small"
    d = dev(fixture_case(fx, name))
    logits = d["logits"].clone().requires_grad_()
    loss = loss_function.detector_loss(d["keypoint_map"], logits, d["valid_mask"], noise=d["noise"])
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    e = D.grad_error(logits.grad.cpu().numpy(), fx[f"{name}.grad"], fx[f"{name}.den64"])
    print(f"autograd: grad err against the recorded reference gradient {e:.2e} (tol {float(fx['tol_grad']):.2e})")
    assert e <= float(fx["tol_grad"])
    assert D.loss_error(loss.detach().cpu().numpy(), fx[f"{name}.loss"]) <= float(fx["tol_loss"])
    twice = d["logits"].clone().requires_grad_()
    (2 * loss_function.detector_loss(d["keypoint_map"], twice, d["valid_mask"], noise=d["noise"])).backward()
    assert torch.equal(twice.grad, 2 * logits.grad)
    # under no_grad no gradient is asked for: nothing is allocated for it
    asked = []
    real = ops.detector_loss
    monkeypatch.setattr(ops, "detector_loss", lambda *a, **k: asked.append(k.get("want_grad", False)) or real(*a, **k))
    with torch.no_grad():
        quiet = loss_function.detector_loss(d["keypoint_map"], logits, d["valid_mask"], noise=d["noise"])
    assert asked == [False] and not quiet.requires_grad and bits_equal(quiet, loss.detach())
    # noise=None draws torch's uniform numbers: same seed, same loss; the draw is the tie-break only
    torch.manual_seed(5)
    a = loss_function.detector_loss(d["keypoint_map"], d["logits"], d["valid_mask"])
    torch.manual_seed(5)
    b = loss_function.detector_loss(d["keypoint_map"], d["logits"], d["valid_mask"])
    assert bits_equal(a, b) and torch.isfinite(a)


def test_guard_bands_stale_workspace_and_unaligned_maps():
    b, hc, wc = 2, 9, 15
    c = D.make_case((b, hc, wc), 31)
    want = run_all(c)
    d = dev(c)
    lib = _lib.lib()
    nbytes = lib.balf_detector_loss_workspace_bytes(b, hc, wc)
    pad = 67                                                                  # (odd: the outputs are not 16-byte aligned)
    sizes = {"loss": 1, "per_image": b, "labels": b * hc * wc, "dlogits": b * 65 * hc * wc}
    stream = _lib.current_stream_ptr(torch.device(DEV))

    def call(kp, vm, outs, ws):
        def at(k):
            return outs[k].data_ptr() + 4 * pad if k in outs else None
        _lib.check(lib.balf_detector_loss(d["logits"].data_ptr(), kp.data_ptr(), vm.data_ptr(), d["noise"].data_ptr(), b, hc, wc,
                                          at("loss"), at("per_image"), at("labels"), at("dlogits"), ws.data_ptr() + 256,
                                          nbytes, stream), "balf_detector_loss")

    def bands():
        return {k: torch.full((n + 2 * pad,), -7, dtype=torch.int32 if k == "labels" else torch.float32, device=DEV)
                for k, n in sizes.items()}

    ws = torch.full((nbytes // 4 + 128,), float("nan"), dtype=torch.float32, device=DEV)      # stale: NaN everywhere
    outs = bands()
    call(d["keypoint_map"], d["valid_mask"], outs, ws)
    for k, n in sizes.items():
        assert bool((outs[k][:pad] == -7).all()) and bool((outs[k][pad + n:] == -7).all()), k
        assert bits_equal(outs[k][pad:pad + n], getattr(want, k).reshape(-1)), k
    assert bool(torch.isnan(ws[:64]).all()) and bool(torch.isnan(ws[64 + nbytes // 4:]).all())
    # want_* off: nothing but the loss is written
    outs = bands()
    call(d["keypoint_map"], d["valid_mask"], {"loss": outs["loss"]}, ws)
    assert bits_equal(outs["loss"][pad:pad + 1], want.loss.reshape(-1))
    for k in ("per_image", "labels", "dlogits"):
        assert bool((outs[k] == -7).all()), k
    # maps that are only 4-byte aligned take the 4-byte loads: same results
    shifted = {}
    for k in ("keypoint_map", "valid_mask"):
        buf = torch.zeros((d[k].numel() + 1,), device=DEV)
        shifted[k] = buf[1:].view(d[k].shape).copy_(d[k])
        assert shifted[k].data_ptr() % 16 == 4 and shifted[k].is_contiguous()
    got = ops.detector_loss(d["logits"], shifted["keypoint_map"], shifted["valid_mask"], d["noise"], want_per_image=True,
                            want_labels=True, want_grad=True)
    for a, w in zip(got, want):
        assert bits_equal(a, w)


def test_graph_capture():
    cases = [D.make_case((2, 9, 15), 40 + i, last_masked=False) for i in range(3)]
    static = dev(cases[0])

    def run(c):
        return ops.detector_loss(c["logits"], c["keypoint_map"], c["valid_mask"], c["noise"], want_per_image=True,
                                 want_labels=True, want_grad=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        outs = run(static)
    for c in (cases[1], cases[2]):
        for k, v in c.items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run(dev(c))
        torch.cuda.synchronize()
        for a, w in zip(outs, want):
            assert bits_equal(a, w)


def test_check_val_anchor_loss(fx):
    hom = {"perspective": 0.2, "rotation": 25, "scale": 0.1}
    ims, labels = [], []
    for i in range(5):
        h, w = ((200, 264), (192, 256))[i % 2]
        gray = synth.synthetic_gray_u8(h, w, 40 + i)
        ims.append(np.ascontiguousarray(np.stack([gray, gray, gray], axis=2)))
        labels.append(S.make_labels("uniform", 60, (h, w), 300 + i))
    loader = SyntheticPairs(ims, labels, hom, 128, 30, 11, batch_pairs=2, device=DEV)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(3))
    model = model.eval().to(DEV)
    got = train_utils.check_val_anchor_loss(loader, model, DEV)
    assert isinstance(got, float)
    want, points = [], 0
    with torch.no_grad():
        for batch in loader:
            v = 0.0
            for images, heat in ((batch[0], batch[2]), (batch[1], batch[3])):
                logits = model(images, want_logits=True)["logits"]
                v += float(D.restate64(logits.cpu(), heat.cpu(), None, None)["loss"])
                points += int(heat.sum())
            want.append(v)
    assert len(want) == 5 and points > 0
    e = D.loss_error(got, np.mean(want))
    print(f"check_val_anchor_loss {got:.7f}, restatement {np.mean(want):.7f}, err {e:.2e} (tol {float(fx['tol_loss']):.2e})")
    assert e <= float(fx["tol_loss"])
    one = train_utils.check_val_anchor_loss(loader, model, DEV, chunk_pairs=1)
    assert np.float64(one).view(np.uint64) == np.float64(got).view(np.uint64)          # independent of chunk_pairs, bit for bit
