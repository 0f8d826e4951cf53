"""balf_amd.optim.FusedAdam / FusedSGD across a training run's life, on the real kernel: the scenarios of
tests/test_optim_life_host.py in which a device pointer changes (``p.data`` or a moment replaced, a list entry replaced, a group
added, 70 parameters, save / load / resume) under the same two oracles (``optim_common.Trio``: the plan-free twin bit for bit,
torch.optim.Adam(foreach=False) / SGD on the device under the float64 gate) -- a stale pointer shows as a new tensor that keeps
its bits or an old one that moves, and both are asserted --; a step issued behind a busy side stream; the refusal of a step inside
a graph capture; and a real run of ``train_head`` over all of stage 4 that is checkpointed and resumed in the reference's order
(train.py: ``ckpt_state`` with ``epoch = cur_epoch + 1`` BEFORE that epoch's ``scheduler.step()``, ``last_epoch = epoch - 1`` on
resuming) against the same run uninterrupted, bit for bit."""
import io
import time

import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.datasets.synthetic_pairs import SyntheticPairs
from balf_amd.model import get_model
from balf_amd.model.stage4_train import TrainableStage4
from balf_amd.optim import FusedAdam, FusedSGD
from balf_amd.utils import synth, train_utils
from tests import optim_common as OC
from tests import pair_synth_common as S
from tests.optim_common import bits_equal, flat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("adam", "sgd")


class Calls:
    """``optim_common.Trio``'s ``kernel``: the sizes of the launches of the optimiser that is stepping."""

    def __init__(self):
        self.opt, self.calls = None, []


@pytest.fixture
def calls(monkeypatch):
    assert _lib.lib().balf_optim_chunk_elems() == OC.CHUNK
    c = Calls()
    real = {"adam_step": ops.adam_step, "sgd_step": ops.sgd_step}

    def counted(name):
        def call(params, *a, **kw):
            c.calls.append(len(params))
            return real[name](params, *a, **kw)
        return call

    for name in real:
        monkeypatch.setattr(ops, name, counted(name))
    return c


def new_param(shape, seed):
    return OC.new_param(shape, seed, DEV)


def same(a, b):
    return bits_equal(a, b) if a.dtype == torch.float32 else (a.dtype == b.dtype and torch.equal(a, b))


# ---- 1. a device pointer changes under the plan ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_data_swapped_between_steps(calls, kind):
    trio = OC.Trio(calls, kind, DEV)
    trio.steps(3)
    olds = [[p.data for p in flat(opt)] for opt in trio.opts]         # (alive: their memory is not handed out again)
    bits = [[t.clone() for t in ts] for ts in olds]

    def mutate(opt):
        for p in flat(opt):
            p.data = p.data.clone()

    trio.each(mutate)
    trio.steps(3)                                                     # (the new tensors moved: the gate, and the twin)
    torch.cuda.synchronize()
    for opt, ts, was in zip(trio.opts, olds, bits):
        assert all(p.data_ptr() != t.data_ptr() for p, t in zip(flat(opt), ts))
        assert all(bits_equal(t, w) for t, w in zip(ts, was))         # the old ones did not


def test_moment_replaced_by_a_clone(calls):
    def mutate(opt):
        ps = flat(opt)
        old = opt.state[ps[2]]["exp_avg"], opt.state[ps[3]]["exp_avg_sq"]
        opt.state[ps[2]]["exp_avg"], opt.state[ps[3]]["exp_avg_sq"] = old[0].clone(), old[1].clone()
        return [t.clone() for t in old], old

    trio, out = OC.life(calls, "adam", DEV, mutate)
    for opt, (was, old) in zip(trio.opts, out):
        ps = flat(opt)
        assert bits_equal(was[0], old[0]) and bits_equal(was[1], old[1])           # the tensors that left the state keep their bits
        assert not bits_equal(opt.state[ps[2]]["exp_avg"], was[0]) and not bits_equal(opt.state[ps[3]]["exp_avg_sq"], was[1])


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_replaced_in_place_in_the_list(calls, kind):
    """``group['params'][i] = new_p``: the new parameter is stepped from state at step 0; the old one and its state keep their bits."""
    def mutate(opt):
        olds = []
        for gi, i, shape, seed in ((0, 1, (65,), 4), (1, 0, (OC.CHUNK + 1,), 5)):
            ps = opt.param_groups[gi]["params"]
            olds.append((ps[i], ps[i].detach().clone(), {k: v.clone() for k, v in opt.state.get(ps[i], {}).items()}))
            ps[i] = new_param(shape, seed)
        return olds

    trio = OC.Trio(calls, kind, DEV)
    trio.steps(3)
    out = trio.each(mutate)
    news = [[flat(opt)[i].detach().clone() for i in (1, 3)] for opt in trio.opts]
    trio.steps(3)
    for opt, olds, was in zip(trio.opts, out, news):
        assert not bits_equal(flat(opt)[1].detach(), was[0]) and not bits_equal(flat(opt)[3].detach(), was[1])
        for old, bits, state in olds:
            assert bits_equal(old.detach(), bits) and all(old is not p for p in flat(opt))
            st = opt.state.get(old, {})
            assert set(st) == set(state) and all(same(st[k], state[k]) for k in state)
    if kind == "adam":
        assert trio.counts() == [6.0, 3.0, 6.0, 3.0, 6.0] and len(trio.fused.state) == len(trio.torch.state) == 7


@pytest.mark.parametrize("kind", KINDS)
def test_add_param_group_after_three_steps(calls, kind):
    def mutate(opt):
        opt.add_param_group({"params": [new_param((300,), 1), new_param((OC.CHUNK + 1,), 2)], "lr": 2e-3})
        return [p.detach().clone() for p in flat(opt)[5:]]

    trio, out = OC.life(calls, kind, DEV, mutate)
    assert len(flat(trio.fused)) == 7 and trio.calls["fused"] == [3, 2, 2]
    for opt, was in zip(trio.opts, out):
        assert all(not bits_equal(p.detach(), w) for p, w in zip(flat(opt)[5:], was))
    if kind == "adam":
        assert trio.counts() == [6.0] * 5 + [3.0] * 2


@pytest.mark.parametrize("kind", KINDS)
def test_seventy_parameters_in_one_group(calls, kind):
    trio = OC.Trio(calls, kind, DEV, OC.seventy(kind, DEV))
    start = [p.detach().clone() for p in flat(trio.fused)]
    for _ in range(3):
        trio.step()
        assert trio.calls["fused"] == [64, 6] and trio.calls["plan-free"] == [64, 6]
    assert all(not bits_equal(p.detach(), w) for p, w in zip(flat(trio.fused), start))
    if kind == "adam":
        assert trio.counts() == [3.0] * 70


def test_save_load_resume_is_the_uninterrupted_run(calls):
    """As on the host: position 4 is a step behind, the state goes through torch.save / torch.load into a fresh instance on cloned
    parameters, and three more steps of both on the same gradients give the same bits."""
    trio = OC.Trio(calls, "adam", DEV)
    trio.step(none=(4,))
    trio.steps(2)
    f = io.BytesIO()
    torch.save(trio.fused.state_dict(), f)
    f.seek(0)
    resumed = FusedAdam(OC.groups_of([torch.nn.Parameter(p.detach().clone()) for p in flat(trio.fused)]), lr=1.0)
    resumed.load_state_dict(torch.load(f))
    for _ in range(3):
        trio.step()
        OC.set_grads(resumed, [p.grad for p in flat(trio.fused)])
        resumed.step()
        for i, (p, q) in enumerate(zip(flat(trio.fused), flat(resumed))):
            a, b = trio.fused.state[p], resumed.state[q]
            assert p.data_ptr() != q.data_ptr() and a["exp_avg"].data_ptr() != b["exp_avg"].data_ptr()
            assert bits_equal(p.detach(), q.detach()) and float(a["step"]) == float(b["step"]), i
            assert bits_equal(a["exp_avg"], b["exp_avg"]) and bits_equal(a["exp_avg_sq"], b["exp_avg_sq"]), i
    assert trio.counts(resumed) == [6.0, 6.0, 6.0, 6.0, 5.0]


# ---- 2. behind a busy side stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_step_is_ordered_on_a_busy_side_stream(kind):
    """The gradients are written on a side stream behind ~0.3 s of device time and ``step()`` follows without a host
    synchronisation: it returns while the stream is busy, and the bits are those of the same step on a drained device."""
    make = OC.five_groups(kind, DEV)
    cls = FusedAdam if kind == "adam" else FusedSGD
    busy_opt, drained = cls(make()), cls(make())
    first = OC.fresh_grads(flat(drained), 70, DEV)
    grads = OC.fresh_grads(flat(drained), 71, DEV)
    for opt in (busy_opt, drained):                                   # warm: state, plans, pointers
        OC.set_grads(opt, first)
        opt.step()
    OC.set_grads(drained, grads)
    drained.step()
    torch.cuda.synchronize()
    for p in flat(busy_opt):
        p.grad.zero_()                                                # (what a step on another stream would read)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(6e8))                                   # ~0.3 s of device time
        for p, g in zip(flat(busy_opt), grads):
            p.grad.copy_(g)
        t0 = time.perf_counter()
        busy_opt.step()
        dt = time.perf_counter() - t0
        done.record()
        busy = not done.query()
    torch.cuda.synchronize()
    assert busy, "the side stream had drained when step() returned: it waited for the device"
    assert dt < 0.1, f"step() took {dt * 1e3:.1f} ms of host time behind a busy stream"
    for i, (p, q) in enumerate(zip(flat(busy_opt), flat(drained))):
        assert bits_equal(p.detach(), q.detach()), i
        if kind == "adam":
            a, b = busy_opt.state[p], drained.state[q]
            assert float(a["step"]) == float(b["step"]) == 2.0
            assert bits_equal(a["exp_avg"], b["exp_avg"]) and bits_equal(a["exp_avg_sq"], b["exp_avg_sq"]), i


# ---- 3. a step cannot be captured ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_step_inside_a_capture_is_refused(calls, kind):
    """The step number and lr are launch arguments, so a replay would repeat the captured step: ``step()`` raises RuntimeError
    before any launch, nothing is touched, and the next eager step is right."""
    trio = OC.Trio(calls, kind, DEV)
    trio.steps(2)
    opt = trio.fused
    grads = OC.fresh_grads(flat(opt), 90, DEV)
    OC.set_grads(opt, grads)
    was = [(p.detach().clone(), {k: v.clone() for k, v in opt.state.get(p, {}).items()}) for p in flat(opt)]
    static = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    calls.calls = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no parallel branches
        static.add_(1.0)
        with pytest.raises(RuntimeError, match="launch arguments"):
            opt.step()
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    assert calls.calls == []                                          # refused before any launch
    for p, (bits, state) in zip(flat(opt), was):
        st = opt.state.get(p, {})
        assert bits_equal(p.detach(), bits) and set(st) == set(state) and all(same(st[k], state[k]) for k in state)
    trio.step()                                                       # the next eager step of all three: gated and compared
    if kind == "adam":
        assert trio.counts() == [3.0] * 5


# ---- 4. a real run, checkpointed and resumed ------------------------------------------------------------------------------------------------
EPOCHS = 4
OPTIM_CFG = {"name": "adam", "lr": 1e-3, "weight_decay": 1e-4}
SCHEDULER_CFG = {"name": "linear", "min_lr": 1e-5, "start_epoch": 1}


def set_up(ckpt=None):
    """What train.py sets a run up with, from scratch or from a checkpoint -> (model, head, optimiser, scheduler, first epoch)."""
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    model.load_state_dict(synth.synthetic_state_dict(2))
    model.precision = "fp32"
    model = model.eval().to(DEV)
    head = TrainableStage4.from_model(model)
    opt = train_utils.build_optimizer(head.parameters(), OPTIM_CFG)
    assert type(opt) is FusedAdam
    start_epoch, last_epoch = 0, -1
    if ckpt is not None:
        head.load_state_dict(ckpt["model_state"])
        opt.load_state_dict(ckpt["optimizer_state"])
        start_epoch = ckpt["epoch"]
        last_epoch = start_epoch - 1
    sched = train_utils.build_scheduler(opt, EPOCHS, last_epoch, SCHEDULER_CFG)
    return model, head, opt, sched, start_epoch


def train(run, batches, stop, log, save_at=None):
    """Epochs ``start_epoch .. stop - 1`` in train.py's order -> the checkpoint file written after epoch ``save_at`` (or None)."""
    model, head, opt, sched, start_epoch = run
    saved = None
    for cur_epoch in range(start_epoch, stop):
        lr = opt.param_groups[0]["lr"]
        loss = train_utils.train_head(batches, model, head, opt, DEV, noise=False)
        log.append((cur_epoch, lr, loss))
        if cur_epoch + 1 == save_at:                                  # before this epoch's scheduler.step()
            saved = io.BytesIO()
            torch.save(train_utils.ckpt_state(head, opt, cur_epoch + 1, 0.0), saved)
            saved.seek(0)
        sched.step()
    return saved


def test_resumed_run_is_the_uninterrupted_run():
    images = S.images()
    labels = [S.make_labels("uniform", 600, im.shape[:2], 321 + i) for i, im in enumerate(images)]
    loader = SyntheticPairs(images, labels, {"perspective": 0.1, "rotation": 10, "scale": 0.05}, 64, 0, 5, batch_pairs=1, device=DEV)
    batches = [tuple(t.clone() for t in batch) for batch in loader]
    assert len(batches) == 2 and batches[0][0].shape == (1, 3, 64, 64) and all(float(b[2].sum()) > 50 for b in batches)
    log_a, log_b = [], []
    run_a = set_up()
    train(run_a, batches, EPOCHS, log_a)
    run_b = set_up()
    saved = train(run_b, batches, 2, log_b, save_at=2)
    ckpt = torch.load(saved)
    assert ckpt["epoch"] == 2 and set(ckpt["optimizer_state"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert ckpt["optimizer_state"]["param_groups"][0]["lr"] == 1e-3    # (epoch 1's: saved before the scheduler moved on)
    del run_b
    run_b = set_up(ckpt)
    assert run_b[4] == 2 and run_b[3].last_epoch == 2
    train(run_b, batches, EPOCHS, log_b)
    print("uninterrupted (epoch, lr, loss):", log_a)
    print("resumed       (epoch, lr, loss):", log_b)
    slope = (1e-3 - 1e-5) / EPOCHS
    assert [e for e, _, _ in log_a] == [0, 1, 2, 3] and [lr for _, lr, _ in log_a] == [1e-3, 1e-3, 1e-3 - slope * 1, 1e-3 - slope * 2]
    assert log_a == log_b                                             # the lr used in each epoch and train_head's four values
    assert len({loss for _, _, loss in log_a}) == EPOCHS                 # (it trains: no two epochs have the same loss)
    (model_a, head_a, opt_a, _, _), (model_b, head_b, opt_b, _, _) = run_a, run_b
    state_a, state_b = head_a.state_dict(), head_b.state_dict()
    assert list(state_a) == list(state_b) and any(k.endswith("num_batches_tracked") for k in state_a)
    for k in state_a:
        assert same(state_a[k], state_b[k]), k
    assert int(head_b.mixer.tail.head.norm.num_batches_tracked) == 2 * 2 * EPOCHS       # two sides of two batches per epoch
    params_a, params_b = list(head_a.parameters()), list(head_b.parameters())
    assert len(params_a) == len(params_b) == 44 == len(opt_a.state) == len(opt_b.state)
    for i, (p, q) in enumerate(zip(params_a, params_b)):
        a, b = opt_a.state[p], opt_b.state[q]
        assert float(a["step"]) == float(b["step"]) == 2.0 * EPOCHS, i
        assert bits_equal(a["exp_avg"], b["exp_avg"]) and bits_equal(a["exp_avg_sq"], b["exp_avg_sq"]), i
    head_a.commit(model_a)
    head_b.commit(model_b)
    x = batches[0][0]
    assert bits_equal(model_a.eval()(x)["logits"], model_b.eval()(x)["logits"])
