"""The training-mode head on the GPU (balf_head_train_forward / balf_head_train_backward, ops.head_train_*,
model.head_train.TrainableHead, MLP_MA_DECODER.encode, utils.train_utils.train_head) against tests/golden/head_train.npz -- the
reference's own modules and autograd, recorded by tests/golden/make_head_train_golden.py -- and against the float64 restatement
of tests/head_train_common.py.  Every output T is gated by err(T) = max |T - T64| / S_T <= tol_T = max(4 * d_T, 1.1e-6) with
d_T the reference's own float32 distance from the restatement (head_train_common.restate64 defines the scales S_T)."""
import numpy as np
import pytest
import torch

from balf_amd import arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.head_train import TrainableHead
from balf_amd.utils import synth, train_utils
from tests import head_train_common as H
from tests import pair_synth_common as S
from tests import train_common as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGIT_TOL = 2e-3                # the gate tests/test_forward_gpu.py applies to the logits of the forward
SWEEP = ((1, 1, 2), (2, 1, 1), (1, 3, 5), (1, 8, 8), (1, 5, 13), (2, 7, 9), (3, 24, 24), (2, 23, 37), (4, 32, 32))
# Where the slice geometry changes (tests/test_train_geometry_host.py asserts each figure).  N = 16899: 512 rows per K slice, S = 34
# with a last slice of 3 rows, a last column block of 3 rows, P = 17 row partials.  N = 66049: 1280 rows per slice, S = 52 with a
# last slice of 769 rows (769 mod 16 = 1), column blocks of 80 rows, PC = 826 with a last block of 49 rows, and P = 65: one lane of
# wave_sum_strided takes a second trip through the channel-major partials.  Cases and restatement on the device.
LARGE = T.LARGE_SHAPES["head"]
NAN_BYTE = 0xFF                 # a buffer of these bytes reads as NaN in float32 and in float64


@pytest.fixture(scope="module")
def fx():
    return H.fixture()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def poison_workspace(n):
    """Fill the cached workspace of this stream with NaN bytes: a stale word that is read shows in the results."""
    ops._workspace("head_train", DEV, ops.lib().balf_head_train_workspace_bytes(n)).fill_(NAN_BYTE)


def run(x2, p, dlogits, running, want_prob=True, want_running=True, want_dx2=True, poison=True):
    """One forward and one backward through ops on the device -> dict of device tensors (GATED, prob).  ``poison``: the
    workspace, ``saved`` and dx2 hold NaN bytes before the calls (the other outputs are fresh ``torch.empty`` tensors of ops)."""
    n = x2.numel() // 256
    d = {k: v.to(DEV) for k, v in p.items()}
    x, g = x2.to(DEV), dlogits.to(DEV)
    rm, rv = (running[0].to(DEV).clone(), running[1].to(DEV).clone()) if want_running else (None, None)
    saved = None
    if poison:
        poison_workspace(n)
        saved = torch.full((ops.lib().balf_head_train_saved_bytes(n),), NAN_BYTE, dtype=torch.uint8, device=DEV)
    f = ops.head_train_forward(x, d["w2"], d["b2"], d["wd"], d["bd"], d["gamma"], d["beta"], eps=H.EPS, want_prob=want_prob,
                               running_mean=rm, running_var=rv, momentum=H.MOMENTUM, saved=saved)
    if poison:
        poison_workspace(n)
    dx2 = want_dx2
    if want_dx2 is True and poison:
        dx2 = torch.full(x.shape, float("nan"), device=DEV)
    b = ops.head_train_backward(g, x, d["w2"], d["wd"], d["gamma"], f.saved, want_dx2=dx2)
    torch.cuda.synchronize()
    out = {"logits": f.logits, "prob": f.prob, "running_mean": rm, "running_var": rv}
    out.update({k: getattr(b, k) for k in H.GRADS})
    return out


def check_against(out, r, fx, what, names=H.GATED):
    errs = {k: H.err(out[k], r[k], r["S"][k]) for k in names if out.get(k) is not None}
    print(what, " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert np.isfinite(e) and e <= float(fx[f"tol_{k}"]), (what, k, e, float(fx[f"tol_{k}"]))
    if out.get("prob") is not None:
        # softmax is 2-Lipschitz in the largest logit error; exp and the division add a few float32 roundings of values <= 1
        e = float((out["prob"].double().to(r["prob"].device) - r["prob"]).abs().max())
        print(what, f"prob {e:.2e}")
        assert e <= 2 * float(fx["tol_logits"]) * r["S"]["logits"] + 4e-7, (what, "prob", e)
    return errs


@pytest.mark.parametrize("name", H.FIXTURE_CASES)
def test_fixture_parity(fx, name):
    x2, p, dlogits, running = H.fixture_case(fx, name)
    r = H.restate64(x2, p, dlogits, running=running)
    out = run(x2, p, dlogits, running)
    check_against(out, r, fx, name)
    if name == "edges":
        c = H.EDGES_GAMMA0                                      # gamma = 0: the logits say nothing about xhat there, dgamma does
        assert float(r["dgamma"][c].abs()) > 1e-3 * r["S"]["dgamma"]
        assert abs(float(out["dgamma"][c]) - float(r["dgamma"][c])) <= float(fx["tol_dgamma"]) * r["S"]["dgamma"]
        assert bool((out["logits"][:, c] == p["beta"][c].to(DEV)).all())
        c = H.EDGES_SHIFTED                                     # mean^2 >> var: xhat of that channel, through its logits
        e = float((out["logits"][:, c].double().cpu() - r["logits"][:, c]).abs().max()) / r["S"]["logits"]
        assert e <= float(fx["tol_logits"]), e
        # h == 0 exactly on channels 0..7 of two rows: dh = 0 there.  db2 of those channels tells: the sum with those two
        # elements let through (the derivative taken as 1 at 0) lies far outside the gate
        h = r["h"].reshape(-1, 256)
        da = r["dz"] @ p["wd"].double()
        wrong = (da * (h >= 0)).sum(0)
        tol = float(fx["tol_db2"]) * r["S"]["db2"]
        got = out["db2"].double().cpu()
        assert float((got[:8] - r["db2"][:8]).abs().max()) <= tol < 0.1 * float((wrong[:8] - r["db2"][:8]).abs().min())


@pytest.mark.parametrize("name", H.FIXTURE_CASES)
def test_autograd_path_against_the_reference(fx, name):
    x2, p, dlogits, running = H.fixture_case(fx, name)
    r = H.restate64(x2, p, dlogits, running=running)
    head = TrainableHead().to(DEV)
    with torch.no_grad():
        for k, t in zip(H.PARAMS, (head.conv2.weight, head.conv2.bias, head.dense.weight, head.dense.bias, head.norm.weight,
                                   head.norm.bias)):
            t.copy_(p[k])
        head.norm.running_mean.copy_(running[0])
        head.norm.running_var.copy_(running[1])
    feat = x2.to(DEV).requires_grad_()
    out = head(feat)
    assert out["logits"].grad_fn is not None and not out["prob"].requires_grad
    (out["logits"] * dlogits.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"logits": out["logits"], "dw2": head.conv2.weight.grad, "db2": head.conv2.bias.grad, "dwd": head.dense.weight.grad,
           "dbd": head.dense.bias.grad, "dgamma": head.norm.weight.grad, "dbeta": head.norm.bias.grad, "dx2": feat.grad,
           "running_mean": head.norm.running_mean, "running_var": head.norm.running_var}
    for k in H.GATED:                                           # against the recorded REFERENCE, in the restatement's scales
        e = H.err(got[k], torch.from_numpy(fx[f"{name}.{k}"]), r["S"][k])
        print(name, k, f"{e:.2e}")
        assert e <= float(fx[f"tol_{k}"]), (k, e)
    assert int(head.norm.num_batches_tracked) == 1
    # no gradient wanted for the features: dx2 is not asked for, the parameter gradients are the same bits
    head.zero_grad()
    (head(x2.to(DEV))["logits"] * dlogits.to(DEV)).sum().backward()
    assert bits_equal(head.conv2.weight.grad, got["dw2"]) and bits_equal(head.norm.weight.grad, got["dgamma"])
    assert int(head.norm.num_batches_tracked) == 2
    with torch.no_grad():
        assert head(x2.to(DEV))["logits"].grad_fn is None and int(head.norm.num_batches_tracked) == 3


_LARGEST = {}


def largest():
    """The last case of LARGE on the device and its first run, made once -> (case, outputs)."""
    if not _LARGEST:
        shape = LARGE[-1]
        c = H.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        _LARGEST.update(case=c, out=run(*c))
    return _LARGEST["case"], _LARGEST["out"]


@pytest.mark.parametrize("shape", SWEEP + LARGE, ids=lambda s: "x".join(map(str, s)))
def test_shape_sweep(fx, shape):
    if shape not in LARGE:
        x2, p, dlogits, running = H.sweep_case(shape, 7 + shape[1] * 100 + shape[2])
        r = H.restate64(x2, p, dlogits, running=running)
        check_against(run(x2, p, dlogits, running), r, fx, str(shape))
        return
    # the same gates with the case and the float64 restatement on the device
    if shape == LARGE[-1]:
        (x2, p, dlogits, running), out = largest()
    else:
        x2, p, dlogits, running = H.sweep_case(shape, 7 + shape[1] * 100 + shape[2], device=DEV)
        out = run(x2, p, dlogits, running)
    r = H.restate64(x2, p, dlogits, running=running)
    # the float32 composition on the CPU, where its three products take under a second: F.batch_norm of torch 2.10 / ROCm 7.0 on the
    # device ended the process (a segmentation fault inside torch) at [1, 65, 257, 257], and the figure needs no device
    cx2, cp, cg, (rm, rv) = T.to_device((x2, p, dlogits, (running[0].clone(), running[1].clone())), torch.device("cpu"))
    logits, grads = H.compose_f32(cx2, cp, cg, running=(rm, rv))
    T.composition_figures(str(shape), dict(grads, logits=logits, running_mean=rm, running_var=rv), r, H.GATED)
    check_against(out, r, fx, str(shape))


def test_largest_shape_gives_the_same_bits_again():
    """The fixed summation order over more than 64 partials per channel, PC = 826 column blocks and S = 52 slabs."""
    c, a = largest()
    b = run(*c)
    for k in H.GATED + ("prob",):
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_bitwise_repeatability():
    c = H.sweep_case((2, 23, 37), 50)
    a, b = run(*c), run(*c)
    for k in H.GATED + ("prob",):
        assert bits_equal(a[k], b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k


def test_independence_of_requests():
    c = H.sweep_case((2, 23, 37), 51)
    full = run(*c)
    lean = run(*c, want_prob=False, want_running=False, want_dx2=False)
    assert lean["prob"] is None and lean["dx2"] is None and lean["running_mean"] is None
    for k in ("logits", "dw2", "db2", "dwd", "dbd", "dgamma", "dbeta"):
        assert bits_equal(full[k], lean[k]), k
    # dx2 into a view that starts 4 bytes into its buffer
    buf = torch.full((c[0].numel() + 1,), float("nan"), device=DEV)
    view = buf[1:].view(c[0].shape)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    off = run(*c, want_dx2=view)
    assert off["dx2"] is view and bits_equal(view, full["dx2"]) and bool(torch.isnan(buf[0]))
    for k in ("logits", "dw2", "dgamma"):
        assert bits_equal(full[k], off[k]), k
    # prob into a view that is not 16-byte aligned: the kernel's 4-byte stores instead of its 16-byte ones, same bits
    pbuf = torch.full((full["prob"].numel() + 2,), float("nan"), device=DEV)
    pview = pbuf[1:-1].view(full["prob"].shape)
    assert pview.data_ptr() % 16 == 4 and pview.is_contiguous()
    off = run(*c, want_prob=pview, want_dx2=False)
    assert off["prob"] is pview and bits_equal(pview, full["prob"]) and bool(torch.isnan(pbuf[0])) and bool(torch.isnan(pbuf[-1]))
    assert bits_equal(full["logits"], off["logits"])


def test_graph_capture():
    shape = (2, 7, 9)
    cases = [H.sweep_case(shape, 60 + i) for i in range(3)]
    x2, p, dlogits, running = cases[0]
    static = {"x2": x2.to(DEV), "g": dlogits.to(DEV), "rm": running[0].to(DEV), "rv": running[1].to(DEV),
              **{k: v.to(DEV) for k, v in p.items()}}

    def step():
        s = static
        f = ops.head_train_forward(s["x2"], s["w2"], s["b2"], s["wd"], s["bd"], s["gamma"], s["beta"], running_mean=s["rm"],
                                   running_var=s["rv"])
        b = ops.head_train_backward(s["g"], s["x2"], s["w2"], s["wd"], s["gamma"], f.saved, want_dx2=True)
        return (f.logits, f.prob) + tuple(b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        outs = step()
    for x2, p, dlogits, running in cases[1:]:
        for k, v in dict(p, x2=x2, g=dlogits, rm=running[0], rv=running[1]).items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run(x2, p, dlogits, running, poison=False)
        assert bits_equal(outs[0], want["logits"]) and bits_equal(outs[1], want["prob"])
        for a, k in zip(outs[2:], H.GRADS):
            assert bits_equal(a, want[k]), k
        assert bits_equal(static["rm"], want["running_mean"]) and bits_equal(static["rv"], want["running_var"])


def synthetic_model(seed, precision):
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(seed))
    model.precision = precision
    return model.eval().to(DEV)


def test_eval_mode(fx):
    x2, p, dlogits, running = H.fixture_case(fx, "edges")
    r = H.restate64(x2, p, stats=torch.stack(running))
    head = TrainableHead().to(DEV)
    with torch.no_grad():
        for k, t in zip(H.PARAMS, (head.conv2.weight, head.conv2.bias, head.dense.weight, head.dense.bias, head.norm.weight,
                                   head.norm.bias)):
            t.copy_(p[k])
        head.norm.running_mean.copy_(running[0])
        head.norm.running_var.copy_(running[1])
    poison_workspace(x2.numel() // 256)
    out = head.eval()(x2.to(DEV).requires_grad_())
    assert out["logits"].grad_fn is None and int(head.norm.num_batches_tracked) == 0
    assert torch.equal(head.norm.running_mean.cpu(), running[0]) and torch.equal(head.norm.running_var.cpu(), running[1])
    check_against(out, r, fx, "eval", names=("logits",))
    assert head(x2.to(DEV), want_prob=False)["prob"] is None


def test_eval_head_on_encoded_features_matches_the_forward():
    model = synthetic_model(3, "fp32")
    g = torch.Generator().manual_seed(9)
    x = torch.rand((2, 3, 128, 192), generator=g).to(DEV)
    want = model(x)
    feat = model.encode(x)
    assert feat.shape == (2, 16, 24, 256) and feat.dtype == torch.float32 and not feat.requires_grad
    got = TrainableHead.from_model(model).eval()(feat)
    e = float((got["logits"] - want["logits"]).abs().max())
    print(f"eval head on encode(x) against forward(x): logits {e:.2e}, prob {float((got['prob'] - want['prob']).abs().max()):.2e}")
    assert e <= LOGIT_TOL
    assert float((got["prob"] - want["prob"]).abs().max()) <= 1e-4          # (the score-map gate of the smoke run)


def test_encode_in_chunks_is_the_concatenation():
    model = synthetic_model(3, "fp32")
    g = torch.Generator().manual_seed(10)
    x = torch.rand((3, 3, 64, 128), generator=g).to(DEV)
    whole = model.encode(x)
    assert bits_equal(whole, torch.cat([model.encode(x[i:i + 1]) for i in range(3)]))
    assert bits_equal(model.encode(x, chunk=2), torch.cat([model.encode(x[:2]), model.encode(x[2:])]))
    assert bits_equal(model.encode(x, chunk=2), whole)          # (the forward is batch-invariant)
    model.train()                                               # the encoder has no training-mode layer; the flag is left alone
    assert bits_equal(model.encode(x), whole) and model.training
    model.eval()


def test_train_head_end_to_end():
    """One pair of 64 x 64 windows with dense labels, presented six times to Adam(lr = 1e-3): few enough pixels (64 a side)
    for the 256-dimensional features to separate them, so that six steps show (probed on the CPU while choosing the chunk:
    the float64 loss fell by 29-37 % over checkpoints 0-5 on such a chunk, 37 % on checkpoint 2)."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    chunk = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(chunk) == 1 and chunk[0][0].shape == (1, 3, 64, 64) and float(chunk[0][2].sum()) > 50
    model = synthetic_model(2, "fp32")
    x = chunk[0][0]
    before = train_utils.check_val_anchor_loss(chunk, model, DEV)
    head = TrainableHead.from_model(model)
    key = model._weights_key(DEV)
    opt = torch.optim.Adam(head.parameters(), lr=1e-3)
    gpu = [train_utils.train_head(chunk, model, head, opt, DEV, noise=False) for _ in range(6)]
    assert model._weights_key(DEV) == key                       # the model was not touched: no re-pack while training
    assert int(head.norm.num_batches_tracked) == 12
    # the same six presentations in float64 on the CPU, from the same features
    feats = [(model.encode(b[0]).cpu(), model.encode(b[1]).cpu(), b[2].cpu(), b[3].cpu()) for b in chunk]
    p, running = H.params_of(synth.synthetic_state_dict(2))
    cpu, _, _ = H.train64(feats, p, running, 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; GPU", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    head.commit(model)
    assert model._weights_key(DEV) != key
    got, want = model.eval()(x)["logits"], head.eval()(model.encode(x))["logits"]
    assert float((got - want).abs().max()) <= LOGIT_TOL
    after = train_utils.check_val_anchor_loss(chunk, model, DEV)
    print(f"check_val_anchor_loss before {before:.4f} after {after:.4f}")
    assert after < before


def test_train_head_with_a_flagged_forward_in_the_chunk_equals_fp32(monkeypatch):
    """A chunk of three batches = six encodes before the guard is asked; the third encode (a saturated image on a re-scaled
    checkpoint, tests/test_forward_gpu.py) leaves the range of the split-f16 path.  Whether the final check finds that flag or
    a later encode of the chunk has consumed it already depends on timing; either way the chunk is encoded again on the fp32
    kernels before any head step, so the epoch equals the fp32 model's bit for bit."""
    import warnings as W
    from tests.golden import cases
    from tests.test_forward_gpu import _scaled_checkpoint_and_images
    sd, bright = _scaled_checkpoint_and_images()
    bright = bright.float().to(DEV)
    calm = cases.forward_input(1, 128, 128, 3).float().to(DEV)
    g = torch.Generator().manual_seed(77)
    heat = [(torch.rand((1, 1, 128, 128), generator=g) < 0.01).float().to(DEV) for _ in range(6)]
    chunk = [(calm, calm.flip(3), heat[0], heat[1]), (bright, calm.flip(2), heat[2], heat[3]), (calm.flip(2), calm, heat[4], heat[5])]

    def model_of(precision):
        m = get_model.load_model(arch.DEFAULT_MODEL_CFG)
        m.load_state_dict(sd)
        m.precision = precision
        return m.eval().to(DEV)

    def epoch(model):
        head = TrainableHead.from_model(model)
        opt = torch.optim.Adam(head.parameters(), lr=1e-3)
        loss = train_utils.train_head(chunk, model, head, opt, DEV, noise=False)
        return loss, head.state_dict()

    want_loss, want = epoch(model_of("fp32"))
    assert np.isfinite(want_loss)
    monkeypatch.delenv("BALF_FP16_STRICT", raising=False)
    monkeypatch.delenv("BALF_FP16_GUARD", raising=False)             # the default: lazy
    m = model_of("fp16")
    with W.catch_warnings():
        W.simplefilter("error")
        m.encode(calm)                                               # probes + an ordinary image: silent, split path
    assert m.effective_precision == "fp16"
    with pytest.warns(RuntimeWarning, match="left the range of its f16 halves"):
        got_loss, got = epoch(m)
    assert m.effective_precision == "fp32"
    assert np.float64(got_loss).view(np.uint64) == np.float64(want_loss).view(np.uint64)
    for k in want:
        assert torch.equal(got[k], want[k]), k
