"""The optimiser step on the GPU (balf_adam_step / balf_sgd_step, ops.adam_step / ops.sgd_step, balf_amd.optim.FusedAdam /
FusedSGD) against the float64 restatement and the bounds of tests/optim_common.py: EVERY element of p', m' and v' within its
bound, at the sizes where the kernel changes path (c = balf_optim_chunk_elems(): one quad, the tail behind it, one chunk, two),
over many tensors in one call, for any cut of the data into tensors and any alignment (identical bits), between guard bands, with
non-finite gradients, through the optimiser classes over several steps and across state dictionaries with torch.optim.Adam, and
in utils.train_utils.train_head."""
import copy

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.head_train import TrainableHead
from balf_amd.optim import FusedAdam, FusedSGD
from balf_amd.utils import synth, train_utils
from tests import head_train_common as H
from tests import optim_common as OC
from tests import pair_synth_common as S
from tests.optim_common import bits_equal
from tests.train_common import Guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYPER = dict(lr=OC.LR, beta1=OC.BETA1, beta2=OC.BETA2, eps=OC.EPS)
SIZES = ("1", "3", "4", "5", "255", "c-1", "c", "c+1", "2c+3")


def chunk():
    return _lib.lib().balf_optim_chunk_elems()


def size(expr):
    return int(eval(expr.replace("2c", "2*c"), {"c": chunk()}))


def dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def adam_once(x, step, wd, **kw):
    """One ops.adam_step on device copies of the float32 arrays x = (p, g, m, v) -> the device tensors (p, g, m, v)."""
    p, g, m, v = dev(x)
    ops.adam_step([p], [g], [m], [v], weight_decay=wd, step=step, **dict(HYPER, **kw))
    return p, g, m, v


# ---- 1. one tensor at the sizes where the kernel changes path ------------------------------------------------------------------------
@pytest.mark.parametrize("numel", SIZES)
def test_one_tensor_adam(numel):
    n = size(numel)
    for wd in (0.0, 0.01):
        for step in (1, 2, 1000):
            x = OC.draw(n, 100 + step, wd)
            p, g, m, v = adam_once(x, step, wd)
            OC.check_adam(f"n={n} wd={wd} step={step}", p, m, v, OC.adam64(*x, step=step, wd=wd))
            assert bits_equal(g, torch.from_numpy(x[1]).to(DEV))


@pytest.mark.parametrize("numel", SIZES)
def test_one_tensor_sgd(numel):
    n = size(numel)
    x = OC.draw(n, 7, 0.0)
    p, g = dev(x[:2])
    ops.sgd_step([p], [g], 1e-2)
    ref = OC.sgd64(x[0], x[1], 1e-2)
    e = OC.excess(p, ref["p"], ref["bp"])
    print(f"sgd n={n}: p' at {e:.3f} of its bound")
    assert e <= 1.0 and bits_equal(g, torch.from_numpy(x[1]).to(DEV))
    assert n < 255 or not bits_equal(p, torch.from_numpy(x[0]).to(DEV))          # (among a few elements lr |g| may round away)


# ---- 2. many tensors in one call ----------------------------------------------------------------------------------------------------
def many(count, wd):
    c = chunk()
    sizes = [(0, 1, 7, 64, 65, c, c + 1)[i % 7] for i in range(count)]
    return sizes, [OC.draw(n, 300 + i, wd) for i, n in enumerate(sizes)]


def test_64_tensors_in_one_call(monkeypatch):
    wd, step = 0.01, 3
    sizes, xs = many(64, wd)
    t = [dev(x) for x in xs]
    grads = [None if i % 5 == 4 else t[i][1] for i in range(64)]
    calls = []
    raw = ops.lib().balf_adam_step
    monkeypatch.setattr(ops.lib(), "balf_adam_step", lambda *a: calls.append(a[0]) or raw(*a))
    ops.adam_step([a[0] for a in t], grads, [a[2] for a in t], [a[3] for a in t], weight_decay=wd, step=step, **HYPER)
    assert calls == [64]                                                       # one library call, hence one launch
    for i, (x, (p, g, m, v)) in enumerate(zip(xs, t)):
        if grads[i] is None or sizes[i] == 0:
            for got, was in ((p, x[0]), (m, x[2]), (v, x[3])):
                assert bits_equal(got, torch.from_numpy(was).to(DEV)), i       # skipped: untouched
        else:
            OC.check_adam(f"tensor {i} n={sizes[i]}", p, m, v, OC.adam64(*x, step=step, wd=wd))


def test_65_tensors_are_split_and_equal_single_calls():
    wd, step = 0.01, 2
    _, xs = many(65, wd)
    together, single = [dev(x) for x in xs], [dev(x) for x in xs]
    ops.adam_step([a[0] for a in together], [a[1] for a in together], [a[2] for a in together], [a[3] for a in together],
                  weight_decay=wd, step=step, **HYPER)
    for p, g, m, v in single:
        if p.numel():
            ops.adam_step([p], [g], [m], [v], weight_decay=wd, step=step, **HYPER)
    for i, (a, b) in enumerate(zip(together, single)):
        for k in (0, 2, 3):
            assert bits_equal(a[k], b[k]), (i, k)
    assert not bits_equal(together[64][0], torch.from_numpy(xs[64][0]).to(DEV))   # the 65th tensor (second call) was stepped
    ps, gs = [a[0].clone() for a in together], [a[1] for a in together]
    ops.sgd_step(ps, gs, 1e-2)
    for i, (p, g, a) in enumerate(zip(ps, gs, together)):
        q = a[0].clone()
        if q.numel():
            ops.sgd_step([q], [g], 1e-2)
        assert bits_equal(p, q), i


# ---- 3. the bits do not depend on how the data is cut into tensors, nor on alignment ----------------------------------------------------
def test_partition_invariance():
    c = chunk()
    n, wd, step = 3 * c + 7, 0.01, 5
    x = OC.draw(n, 500, wd)
    whole = adam_once(x, step, wd)
    assert all(t.data_ptr() % 16 == 0 for t in whole)
    OC.check_adam("whole", whole[0], whole[2], whole[3], OC.adam64(*x, step=step, wd=wd))
    cuts = (0, 1, c - 2, c + 3, 2 * c + 5, n)
    # p, g, m, v each in a buffer of its own, started 0, 1, 2 and 3 floats behind a 16-byte boundary: the four pointers of a piece
    # are 4-byte aligned and differ from one another in alignment
    flat = []
    for k, a in enumerate(x):
        buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[k:k + n] = torch.from_numpy(a).to(DEV)
        flat.append(buf[k:k + n])
    pieces = [[f[a:b] for a, b in zip(cuts[:-1], cuts[1:])] for f in flat]
    assert len(pieces[0]) == 5 and all(t.is_contiguous() for s in pieces for t in s)
    assert len({t.data_ptr() % 16 for t in (pieces[0][1], pieces[1][1], pieces[2][1], pieces[3][1])}) == 4
    ops.adam_step(pieces[0], pieces[1], pieces[2], pieces[3], weight_decay=wd, step=step, **HYPER)
    for k in (0, 2, 3):
        assert bits_equal(flat[k], whole[k]), ("p", "g", "m", "v")[k]
    assert bits_equal(flat[1], whole[1])
    # SGD likewise
    p_whole, p_flat = dev([x[0]])[0], torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    p_flat[1:n + 1] = p_whole
    ops.sgd_step([p_whole], [whole[1]], 1e-2)
    ops.sgd_step([p_flat[1:n + 1][a:b] for a, b in zip(cuts[:-1], cuts[1:])], pieces[1], 1e-2)
    assert bits_equal(p_flat[1:n + 1], p_whole)


# ---- 4. guard bands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (0, 4))
@pytest.mark.parametrize("numel", ("5", "c+1", "2c+3"))
def test_guard_bands(numel, offset):
    """p, g, m and v of exactly numel floats each between two 1 MiB bands of pattern, starting on a 256-byte boundary or 4 bytes
    behind one: both entry points leave every band intact and do not write g."""
    n, wd, step = size(numel), 0.01, 4
    x = OC.draw(n, 700, wd)
    bufs = [Guarded.of(t, offset=offset) for t in dev(x)]
    p, g, m, v = (b.view(torch.float32, (n,)) for b in bufs)
    assert p.data_ptr() % 256 == offset
    ops.adam_step([p], [g], [m], [v], weight_decay=wd, step=step, **HYPER)
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    assert bits_equal(g, torch.from_numpy(x[1]).to(DEV))
    OC.check_adam(f"guarded n={n} offset={offset}", p, m, v, OC.adam64(*x, step=step, wd=wd))
    bufs[0].load(dev([x[0]])[0])
    ops.sgd_step([p], [g], 1e-2)
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    assert bits_equal(g, torch.from_numpy(x[1]).to(DEV))
    ref = OC.sgd64(x[0], x[1], 1e-2)
    assert OC.excess(p, ref["p"], ref["bp"]) <= 1.0


# ---- 5. non-finite gradients stay where they are ---------------------------------------------------------------------------------------
def test_nan_and_inf_gradients():
    c = chunk()
    n, wd, step = c + 1, 0.01, 2
    x = OC.draw(n, 900, wd)
    at_nan, at_inf = 7, c                                       # one in a quad of the vector path, one the tail element
    x[1][at_nan], x[1][at_inf] = np.nan, -np.inf
    p, g, m, v = adam_once(x, step, wd)
    ref = OC.adam64(*x, step=step, wd=wd)
    keep = np.ones(n, bool)
    keep[[at_nan, at_inf]] = False
    for k, t in (("p", p), ("m", m), ("v", v)):
        got = t.cpu().numpy()
        for at in (at_nan, at_inf):
            want = ref[k][at]
            assert not np.isfinite(want)
            assert (np.isnan(got[at]) and np.isnan(want)) or got[at] == want, (k, at, got[at], want)
        assert np.isfinite(got[keep]).all(), k
    assert np.isnan(ref["p"][at_inf]) and ref["m"][at_inf] == -np.inf and ref["v"][at_inf] == np.inf
    OC.check_adam("finite elements", p, m, v, ref, keep=keep)


# ---- 6. the optimiser classes over several steps ----------------------------------------------------------------------------------------
def five_params(seed=11):
    return OC.five_params(DEV, seed, chunk())


def fresh_grads(params, seed):
    return OC.fresh_grads(params, seed, DEV)


groups_of, snapshot, gate_step, set_grads = OC.groups_of, OC.snapshot, OC.gate_step, OC.set_grads


def test_fused_adam_six_steps_and_torch_under_the_same_gate():
    fused = FusedAdam(groups_of(five_params()))
    ours = torch.optim.Adam(groups_of(five_params()), foreach=False)
    flat = [p for grp in fused.param_groups for p in grp["params"]]
    for k in range(6):
        grads = fresh_grads(flat, 40 + k)
        for name, opt in (("FusedAdam", fused), ("torch Adam(foreach=False)", ours)):
            before = snapshot(opt)
            set_grads(opt, grads)
            opt.step()
            gate_step(f"{name} step {k + 1}", opt, before, grads)
    # the moments of a group are views of one arena each, every view on a 16-byte boundary
    for grp in fused.param_groups:
        ms = [fused.state[p]["exp_avg"] for p in grp["params"]]
        assert len({m.untyped_storage().data_ptr() for m in ms}) == 1 and all(m.data_ptr() % 16 == 0 for m in ms)
    # a changed lr takes effect at the next step
    fused.param_groups[1]["lr"] = 5e-4
    grads = fresh_grads(flat, 60)
    before = snapshot(fused)
    set_grads(fused, grads)
    fused.step()
    gate_step("lr 5e-4", fused, before, grads)
    p3 = fused.param_groups[1]["params"][0]
    wrong = OC.adam64(before[3][0], grads[3].cpu().numpy().reshape(-1), before[3][1], before[3][2], step=before[3][3] + 1, wd=0.01, lr=3e-3)
    assert OC.excess(p3.detach(), wrong["p"], wrong["bp"]) > 1.0                   # (the old lr would not pass)
    # lr = 0 with wd = 0: p keeps its bits, m, v and step advance; a parameter without a gradient keeps bits and step
    fused.param_groups[0]["lr"] = 0.0
    grads = fresh_grads(flat, 61)
    grads[4] = None
    before = snapshot(fused)
    set_grads(fused, grads)
    fused.step()
    gate_step("lr 0", fused, before, grads)
    for i, p in enumerate(fused.param_groups[0]["params"]):
        st = fused.state[p]
        assert bits_equal(p.detach().reshape(-1), torch.from_numpy(before[i][0]).to(DEV)), i
        assert not bits_equal(st["exp_avg"].reshape(-1), torch.from_numpy(before[i][1]).to(DEV)) and int(st["step"]) == 8
    p4 = fused.param_groups[1]["params"][1]
    assert int(fused.state[p4]["step"]) == 7 and bits_equal(fused.state[p4]["exp_avg"].reshape(-1), torch.from_numpy(before[4][1]).to(DEV))
    # the next step partitions by step value (7 and 8 in group 1) and still steps every tensor correctly
    grads = fresh_grads(flat, 62)
    before = snapshot(fused)
    set_grads(fused, grads)
    fused.step()
    gate_step("mixed step counts", fused, before, grads)
    assert int(fused.state[p4]["step"]) == 8 and int(fused.state[p3]["step"]) == 9


def test_fused_sgd_and_schedulers():
    params = five_params(12)
    opt = FusedSGD(groups_of(params)[0]["params"] + groups_of(params)[1]["params"], lr=1e-2)
    sched = train_utils.build_scheduler(opt, 10, -1, {"name": "linear", "min_lr": 0.0, "start_epoch": 0})
    for k in range(3):
        grads = fresh_grads(params, 80 + k)
        before = [p.detach().cpu().numpy().reshape(-1).copy() for p in params]
        set_grads(opt, grads)
        lr = opt.param_groups[0]["lr"]
        assert lr == pytest.approx(1e-2 * (1 - k / 10))
        opt.step()
        for p, p0, g in zip(params, before, grads):
            ref = OC.sgd64(p0, g.cpu().numpy().reshape(-1), lr)
            assert OC.excess(p.detach(), ref["p"], ref["bp"]) <= 1.0
        sched.step()


# ---- 7. state dictionaries, both ways ------------------------------------------------------------------------------------------------------
def test_state_dict_from_and_to_torch_adam():
    shapes = ((1,), (65,), (33, 65), (chunk() + 1,))
    gen = torch.Generator().manual_seed(5)
    cpu = [torch.nn.Parameter(0.1 * torch.randn(s, generator=gen)) for s in shapes]
    theirs = torch.optim.Adam(cpu, lr=2e-3, weight_decay=0.01)
    for k in range(3):
        for p, g in zip(cpu, fresh_grads(cpu, 20 + k)):
            p.grad = g.cpu()
        theirs.step()
    gpu = [torch.nn.Parameter(p.detach().to(DEV)) for p in cpu]
    fused = FusedAdam(gpu, lr=1.0)                                      # (every hyper-parameter comes from the loaded groups)
    fused.load_state_dict(theirs.state_dict())
    assert fused.param_groups[0]["lr"] == 2e-3 and fused.param_groups[0]["weight_decay"] == 0.01
    grads = fresh_grads(gpu, 30)
    before = snapshot(fused)
    assert [b[3] for b in before] == [3] * 4
    for b, p in zip(before, cpu):                                       # the loaded moments are the CPU optimiser's, bit for bit
        assert np.array_equal(b[1], theirs.state[p]["exp_avg"].numpy().reshape(-1)) and np.abs(b[2]).max() > 0
    set_grads(fused, grads)
    fused.step()
    gate_step("fourth step after loading torch's state", fused, before, grads)
    # and back: FusedAdam's state_dict in torch.optim.Adam, on the GPU and on the CPU
    sd = copy.deepcopy(fused.state_dict())                              # (as read from a checkpoint: load_state_dict shares tensors)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in gpu]
    back = torch.optim.Adam(twins, lr=1.0, foreach=False)
    back.load_state_dict(copy.deepcopy(sd))
    assert all(int(back.state[p]["step"]) == 4 for p in twins) and back.param_groups[0]["lr"] == 2e-3
    grads = fresh_grads(gpu, 31)
    before = snapshot(back)
    for a, b in zip(before, snapshot(fused)):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    set_grads(back, grads)
    back.step()
    gate_step("torch's fifth step from FusedAdam's state", back, before, grads)
    on_cpu = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu()) for p in gpu], lr=1.0)
    on_cpu.load_state_dict(sd)
    assert all(int(st["step"]) == 4 and st["exp_avg"].device.type == "cpu" for st in on_cpu.state.values())
    ck = train_utils.ckpt_state(torch.nn.Linear(2, 2), fused, 3, 50.0)
    assert set(ck["optimizer_state"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


# ---- 8. what is refused --------------------------------------------------------------------------------------------------------------
def test_refusals():
    good = lambda: [torch.nn.Parameter(torch.randn(4, 6, device=DEV))]          # noqa: E731
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            FusedAdam(good(), **{flag: True})
    with pytest.raises(ValueError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.randn(4, device=DEV, dtype=torch.float64))])
    with pytest.raises(ValueError, match="float32"):
        FusedSGD([torch.nn.Parameter(torch.randn(4, device=DEV, dtype=torch.float16))], lr=0.1)
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.randn(4, 6, device=DEV).t())])
    opt = FusedAdam(good())
    p = opt.param_groups[0]["params"][0]
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 6)).to(DEV)
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    p.grad = torch.ones_like(p)
    was = p.detach().clone()
    with pytest.raises(ValueError, match="requires grad"):
        opt.step(lambda: (p * p).sum())
    assert bits_equal(p.detach(), was) and len(opt.state[p]) == 0                  # refused before anything was stepped
    assert opt.step(lambda: 1.5) == 1.5 and not bits_equal(p.detach(), was)         # a plain closure is fine
    assert float(opt.step(lambda: (p * p).sum().detach())) > 0 and int(opt.state[p]["step"]) == 2
    opt.param_groups[0]["amsgrad"] = True                                         # set behind the constructor's back
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    with pytest.raises(_lib.BalfHipError):
        ops.adam_step([was], [was.double()], [was.clone()], [was.clone()], weight_decay=0.0, step=1, **HYPER)
    with pytest.raises(_lib.BalfHipError):
        ops.adam_step([was], [was[:2]], [was.clone()], [was.clone()], weight_decay=0.0, step=1, **HYPER)
    with pytest.raises(_lib.BalfHipError):
        ops.sgd_step([was], [was.cpu()], 0.1)


def test_build_optimizer_on_gpu_parameters():
    adam = train_utils.build_optimizer(five_params(), {"name": "adam", "lr": 2e-3, "weight_decay": 1e-4})
    assert type(adam) is FusedAdam and adam.param_groups[0]["lr"] == 2e-3 and adam.param_groups[0]["weight_decay"] == 1e-4
    assert adam.param_groups[0]["betas"] == (0.9, 0.999) and adam.param_groups[0]["eps"] == 1e-8
    assert type(train_utils.build_optimizer(five_params(), {"name": "sgd", "lr": 0.1})) is FusedSGD
    mixed = five_params() + [torch.nn.Parameter(torch.zeros(3, device=DEV, dtype=torch.float64))]
    assert type(train_utils.build_optimizer(mixed, {"name": "adam", "lr": 1e-3, "weight_decay": 0})) is torch.optim.Adam


# ---- 9. train_head with FusedAdam ---------------------------------------------------------------------------------------------------
def test_train_head_with_fused_adam(monkeypatch):
    """tests/test_head_train_gpu.py::test_train_head_end_to_end with FusedAdam in torch.optim.Adam's place: the same chunk, the same
    gates, and one library call per step."""
    image = S.images()[0]
    labels = S.make_labels("uniform", 600, image.shape[:2], 321)
    loader = SyntheticPairs([image], [labels], {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1,
                            device=DEV)
    batches = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(batches) == 1 and batches[0][0].shape == (1, 3, 64, 64) and float(batches[0][2].sum()) > 50
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(2))
    model.precision = "fp32"
    model = model.eval().to(DEV)
    head = TrainableHead.from_model(model)
    key = model._weights_key(DEV)
    opt = FusedAdam(head.parameters(), lr=1e-3)
    calls, real = [], ops.adam_step

    def counted(params, *a, **kw):
        calls.append(len(params))
        return real(params, *a, **kw)

    monkeypatch.setattr(ops, "adam_step", counted)
    gpu = [train_utils.train_head(batches, model, head, opt, DEV, noise=False) for _ in range(6)]
    assert calls == [6] * 6                                                       # six steps, one call of six tensors each
    assert all(int(st["step"]) == 6 for st in opt.state.values()) and len(opt.state) == 6
    assert model._weights_key(DEV) == key
    feats = [(model.encode(b[0]).cpu(), model.encode(b[1]).cpu(), b[2].cpu(), b[3].cpu()) for b in batches]
    p, running = H.params_of(synth.synthetic_state_dict(2))
    cpu, _, _ = H.train64(feats, p, running, 6)
    fall_cpu, fall_gpu = 1 - cpu[-1] / cpu[0], 1 - gpu[-1] / gpu[0]
    print("float64", [round(v, 4) for v in cpu], f"fall {fall_cpu:.3f}; FusedAdam", [round(v, 4) for v in gpu], f"fall {fall_gpu:.3f}")
    assert fall_cpu >= 0.30
    assert all(np.isfinite(gpu)) and fall_gpu >= 0.5 * fall_cpu
    head.commit(model)
    assert model._weights_key(DEV) != key
    x = batches[0][0]
    got, want = model.eval()(x)["logits"], head.eval()(model.encode(x))["logits"]
    assert float((got - want).abs().max()) <= 2e-3                                # the gate of test_train_head_end_to_end
