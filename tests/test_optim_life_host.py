"""balf_amd.optim.FusedAdam / FusedSGD across a training run's life, without a GPU: what the per-group plans (cached pointers, runs
keyed by which parameters had a gradient, the CPU tensor of step counts) do when the things they cache change behind their back --
``p.data`` or a moment replaced, the state cleared, popped from or replaced, the group's list grown, copied, or an entry of it
replaced or swapped, more than 64 parameters, more than 64 gradient patterns, state dictionaries saved, loaded and shared, the
optimiser deep-copied or pickled.

The real classes run on CPU tensors.  Of ``_check_param`` only the ``is_cuda`` refusal is lifted, and ``ops.optim_pointers``,
``ops.adam_step``, ``ops.sgd_step`` are replaced by ``Kernel`` below: the kernel's float32 restatement (``optim_common.adam32``;
``p - lr * g`` for SGD), in place, which on EVERY call asserts that the pointers it is handed were gathered from the tensors it is
handed, that the cached element counts are theirs, and that each parameter is, by identity, in its group's current list.

Every scenario is judged by the two oracles of ``optim_common.Trio`` after every step: (a) the plan-free twin, bit for bit; (b) torch's
own optimiser under the same mutation, under the one-step float64 gate, with equal step counts and the same parameters with state."""
import copy
import io
import pickle
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from balf_amd import ops
from balf_amd.optim import FusedAdam, _FusedOptimizer
from tests import optim_common as OC
from tests.optim_common import bits_equal, flat

CPU = torch.device("cpu")
KINDS = ("adam", "sgd")


class Kernel:
    """What stands in for the library.  ``opt``: the optimiser that is being stepped (set by ``Trio.step``)."""

    def __init__(self):
        self.opt, self.calls, self.gathers = None, [], 0

    def optim_pointers(self, params, exp_avgs=None, exp_avg_sqs=None):
        tensors = list(params) + list(exp_avgs or ()) + list(exp_avg_sqs or ())
        assert 1 <= len(params) <= 64 and len(tensors) in (len(params), 3 * len(params))
        for i, t in enumerate(tensors):                               # what the real one refuses
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params[i % len(params)].numel():
                raise ops.OptimArgumentError(f"tensor {i}: {t.dtype}, strides {t.stride()}, {t.numel()} elements")
        self.gathers += 1
        return SimpleNamespace(n=len(params), numels=tuple(p.numel() for p in params), key=tuple(t.data_ptr() for t in tensors),
                               m=exp_avgs)

    def _checked(self, params, tensors, o):
        assert o is not None and o.n == len(params)
        assert o.key == tuple(t.data_ptr() for t in tensors), "the pointers were gathered from other tensors"
        assert o.numels == tuple(p.numel() for p in params), "the cached element counts are not these parameters'"
        home = [grp["params"] for grp in self.opt.param_groups if any(q is params[0] for q in grp["params"])]
        assert len(home) == 1 and all(any(q is p for q in home[0]) for p in params), "a tensor that is not in the group's list"

    def adam_step(self, params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, weight_decay, step, pointers=None):
        self._checked(params, list(params) + list(exp_avgs) + list(exp_avg_sqs), pointers)
        assert len(grads) == len(params) and int(step) >= 1
        self.calls.append(len(params))
        for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
            if g is None:
                continue
            assert g.dtype == torch.float32 and g.shape == p.shape
            a = [t.detach().contiguous().numpy().reshape(-1) for t in (p, g)] + [t.numpy().reshape(-1) for t in (m, v)]
            assert all(np.shares_memory(x, t.detach().numpy()) for x, t in zip(a, (p, g, m, v)))
            a[0][:], a[2][:], a[3][:] = OC.adam32(*a, step=int(step), wd=weight_decay, lr=lr, b1=beta1, b2=beta2, eps=eps)

    def sgd_step(self, params, grads, lr, pointers=None):
        self._checked(params, list(params), pointers)
        assert len(grads) == len(params)
        self.calls.append(len(params))
        for p, g in zip(params, grads):
            if g is not None:
                a = p.detach().numpy().reshape(-1)
                a[:] = a - np.float32(lr) * g.numpy().reshape(-1)


@pytest.fixture
def kernel(monkeypatch):
    real = _FusedOptimizer._check_param.__func__

    def on_any_device(cls, p):
        try:
            real(cls, p)
        except ValueError as e:                                      # (the last of its checks: every other one has passed)
            if "must be on the GPU" not in str(e):
                raise

    k = Kernel()
    monkeypatch.setattr(_FusedOptimizer, "_check_param", classmethod(on_any_device))
    for name in ("optim_pointers", "adam_step", "sgd_step"):
        monkeypatch.setattr(ops, name, getattr(k, name))
    return k


def new_param(shape, seed):
    return OC.new_param(shape, seed, CPU)


def life(kernel, kind, mutate, **kw):
    return OC.life(kernel, kind, CPU, mutate, **kw)


class Trio(OC.Trio):
    def __init__(self, kernel, kind, make=None, opts=None):
        super().__init__(kernel, kind, CPU, make, opts)


# ---- tensors replaced under the plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_data_swapped_between_steps(kernel, kind):
    def mutate(opt):
        for p in flat(opt):
            p.data = p.data.clone()

    trio = Trio(kernel, kind)
    trio.steps(3)
    kept = [p.data for opt in trio.opts for p in flat(opt)]           # (alive, so that no address is used again)
    gathers = kernel.gathers
    trio.each(mutate)
    trio.step()
    assert kernel.gathers == gathers + 2 + 2                          # both groups of both fused instances
    trio.steps(2)
    assert kernel.gathers == gathers + 4 + 2 * 2                      # then only the plan-free twin gathers again
    assert all(p.data_ptr() != old.data_ptr() for p, old in zip(flat(trio.fused), kept))


def test_moment_replaced_by_a_clone(kernel):
    def mutate(opt):
        ps = flat(opt)
        old = opt.state[ps[2]]["exp_avg"], opt.state[ps[3]]["exp_avg_sq"]
        opt.state[ps[2]]["exp_avg"], opt.state[ps[3]]["exp_avg_sq"] = old[0].clone(), old[1].clone()
        return [t.clone() for t in old], old

    trio, out = life(kernel, "adam", mutate)
    for was, old in out:                                              # the tensors that left the state keep their bits
        assert bits_equal(was[0], old[0]) and bits_equal(was[1], old[1])


def test_moment_replaced_by_float64(kernel):
    """``_moment`` converts it once, in the state itself (torch's own class cannot step a float64 moment of a float32 parameter:
    its twin gets the same values in float32)."""
    def mutate(opt):
        st = opt.state[flat(opt)[3]]
        wide = st["exp_avg_sq"].double()
        st["exp_avg_sq"] = wide if isinstance(opt, _FusedOptimizer) else wide.float()

    trio = Trio(kernel, "adam")
    trio.steps(3)
    trio.each(mutate)
    st = trio.fused.state[flat(trio.fused)[3]]
    assert st["exp_avg_sq"].dtype == torch.float64
    trio.step()
    first = st["exp_avg_sq"]
    assert first.dtype == torch.float32 and first.is_contiguous()
    gathers = kernel.gathers
    trio.steps(2)
    assert st["exp_avg_sq"] is first and kernel.gathers == gathers + 2 * 2      # converted once; nothing gathered again for it


def test_moment_replaced_by_a_non_contiguous_one(kernel):
    def mutate(opt):
        st = opt.state[flat(opt)[2]]
        st["exp_avg"] = st["exp_avg"].t().contiguous().t()            # the same values, strides (1, 256)
        assert not st["exp_avg"].is_contiguous()

    trio = Trio(kernel, "adam")
    trio.steps(3)
    trio.each(mutate)
    trio.step()
    st = trio.fused.state[flat(trio.fused)[2]]
    first = st["exp_avg"]
    assert first.is_contiguous() and first.shape == (256, 65)
    trio.steps(2)
    assert st["exp_avg"] is first


# ---- the state cleared, replaced, popped from ------------------------------------------------------------------------------------------
def test_state_cleared(kernel):
    trio, _ = life(kernel, "adam", lambda opt: opt.state.clear())
    assert trio.counts() == [3.0] * 5                                 # every parameter started again at step 0


def test_state_replaced_by_a_new_dictionary(kernel):
    def mutate(opt):
        opt.state = defaultdict(dict)

    trio, _ = life(kernel, "adam", mutate)
    assert trio.counts() == [3.0] * 5


def test_state_popped_of_one_parameter(kernel):
    trio, out = life(kernel, "adam", lambda opt: opt.state.pop(flat(opt)[3]))
    assert trio.counts() == [6.0, 6.0, 6.0, 3.0, 6.0]
    for opt, popped in zip(trio.opts, out):                           # the popped dictionary is nobody's state any more
        assert float(popped["step"]) == 3.0 and opt.state[flat(opt)[3]] is not popped


def test_state_popped_while_another_parameter_gets_its_first_gradient(kernel):
    """Position 2 (group 0) has no gradient, hence no state, for three steps; then position 3 (group 1) is popped and every
    gradient is there.  Group 0 adds the entry that the pop took away before group 1 is looked at: the number of entries is what
    it was after the last step."""
    trio = Trio(kernel, "adam")
    trio.steps(3, none=(2,))
    assert trio.counts() == [3.0, 3.0, None, 3.0, 3.0] and len(trio.fused.state) == 4
    trio.each(lambda opt: opt.state.pop(flat(opt)[3]))
    trio.step()
    assert len(trio.fused.state) == 5 and trio.counts() == [4.0, 4.0, 1.0, 1.0, 4.0]
    trio.steps(2)
    assert trio.counts() == [6.0, 6.0, 3.0, 3.0, 6.0]


# ---- the groups and their lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_add_param_group_after_three_steps(kernel, kind):
    def mutate(opt):
        opt.add_param_group({"params": [new_param((300,), 1), new_param((OC.CHUNK + 1,), 2)], "lr": 2e-3})

    trio, _ = life(kernel, kind, mutate)
    assert len(flat(trio.fused)) == 7 and trio.calls["fused"] == [3, 2, 2]
    if kind == "adam":
        assert trio.counts() == [6.0] * 5 + [3.0] * 2


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_appended_to_a_groups_list(kernel, kind):
    trio, _ = life(kernel, kind, lambda opt: opt.param_groups[0]["params"].append(new_param((OC.CHUNK + 1,), 3)))
    assert trio.calls["fused"][-1] == 2 and len(flat(trio.fused)) == 6
    if kind == "adam":
        assert trio.counts() == [6.0, 6.0, 6.0, 3.0, 6.0, 6.0]        # (two launches for group 0: steps 7 and 4)
        assert trio.calls["fused"] == [3, 1, 2]
    else:
        assert trio.calls["fused"] == [4, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_groups_list_replaced_by_a_copy(kernel, kind):
    def mutate(opt):
        for grp in opt.param_groups:
            grp["params"] = list(grp["params"])

    trio, _ = life(kernel, kind, mutate)
    assert trio.calls["fused"] == [3, 2]
    if kind == "adam":
        assert trio.counts() == [6.0] * 5


@pytest.mark.parametrize("kind", KINDS)
def test_parameter_replaced_in_place_in_the_list(kernel, kind):
    """``group['params'][i] = new_p``: the list is the same object of the same length.  The new parameter is stepped from state at
    step 0, the old one and its state are left alone, as torch does."""
    def mutate(opt):
        olds = []
        for gi, i, shape, seed in ((0, 1, (65,), 4), (1, 0, (OC.CHUNK + 1,), 5)):
            ps = opt.param_groups[gi]["params"]
            olds.append((ps[i], ps[i].detach().clone(), {k: v.clone() for k, v in opt.state.get(ps[i], {}).items()}))
            ps[i] = new_param(shape, seed)
        return olds

    trio = Trio(kernel, kind)
    trio.steps(3)
    out = trio.each(mutate)
    news_before = [flat(opt)[1].detach().clone() for opt in trio.opts]
    trio.steps(3)
    for opt, olds, was in zip(trio.opts, out, news_before):
        assert not bits_equal(flat(opt)[1].detach(), was)             # the new tensor moved ...
        for old, bits, state in olds:                                 # ... and the old one, and its state, did not
            assert bits_equal(old.detach(), bits) and all(old is not p for p in flat(opt))
            st = opt.state.get(old, {})
            assert set(st) == set(state) and all(bits_equal(st[k], state[k]) for k in state)
    if kind == "adam":
        assert trio.counts() == [6.0, 3.0, 6.0, 3.0, 6.0] and len(trio.fused.state) == len(trio.torch.state) == 7


@pytest.mark.parametrize("kind", KINDS)
def test_two_entries_swapped_in_the_list(kernel, kind):
    def mutate(opt):
        ps = opt.param_groups[0]["params"]
        ps[0], ps[2] = ps[2], ps[0]

    # (FusedAdam: unequal step counts, so that the order of the state matters too)
    trio, _ = life(kernel, kind, mutate, none_before=(0,) if kind == "adam" else ())
    assert [p.numel() for p in flat(trio.fused)] == [256 * 65, 65, 1, OC.CHUNK + 1, 3]
    if kind == "adam":
        assert trio.counts() == [6.0, 6.0, 3.0, 6.0, 6.0]


# ---- more than 64 parameters, more than 64 patterns -----------------------------------------------------------------------------------------
def seventy(kind):
    return OC.seventy(kind, CPU)


@pytest.mark.parametrize("kind", KINDS)
def test_seventy_parameters_in_one_group(kernel, kind):
    trio = Trio(kernel, kind, seventy(kind))
    for _ in range(3):
        trio.step()
        assert trio.calls["fused"] == [64, 6] and trio.calls["plan-free"] == [64, 6]
    if kind == "adam":
        assert trio.counts() == [3.0] * 70


@pytest.mark.parametrize("kind", KINDS)
def test_seventy_parameters_with_ragged_gradients(kernel, kind):
    """About 30 % of the gradients are None on the odd steps, so the step counts spread and a run is cut by count and by 64."""
    rng = np.random.default_rng(70)
    trio = Trio(kernel, kind, seventy(kind))
    want = np.zeros(70)
    for k in range(6):
        none = tuple(np.flatnonzero(rng.random(70) < 0.3)) if k % 2 == 0 else ()
        trio.step(none)
        want += 1
        want[list(none)] -= 1
        assert sum(trio.calls["fused"]) == 70 - len(none) and max(trio.calls["fused"]) <= 64
        assert trio.calls["fused"] == trio.calls["plan-free"]
    if kind == "adam":
        assert trio.counts() == list(want) and len(set(want)) >= 3


def test_more_than_64_gradient_patterns(kernel):
    """Eight parameters stepped through 70 distinct patterns of present gradients: the set bits of m, then of its complement, for
    m = 1 .. 35, so that after every pair the step counts are equal again and each step is ONE run, keyed by a set of positions that
    was not seen before.  The plan's runs are dropped once 64 have gathered; the step counts stay torch's after every step
    (``Trio.compare``)."""
    def make():
        shapes = ((1,), (3,), (5,), (17,), (4, 4), (33,), (2, 3), (65,))
        return [{"params": [new_param(s, 200 + i) for i, s in enumerate(shapes)], "lr": 1e-3, "weight_decay": 0.01}]

    trio = Trio(kernel, "adam", make)
    masks = [m ^ flip for m in range(1, 36) for flip in (0, 255)]
    assert len(set(masks)) == 70
    sizes = []
    for mask in masks:
        trio.step(tuple(i for i in range(8) if not mask >> i & 1))
        assert trio.calls["fused"] == [bin(mask).count("1")]
        sizes.append(len(trio.fused._plans[0].runs))
    print("runs held after each step:", sizes)
    assert sizes == list(range(1, 65)) + list(range(1, 7))            # runs.clear() happened at the 65th pattern
    assert trio.counts() == [35.0] * 8


# ---- state dictionaries ---------------------------------------------------------------------------------------------------------------------
def through_a_file(obj):
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f)


def test_save_load_resume_is_the_uninterrupted_run(kernel):
    """Position 4 has its first gradient one step after the others.  After three steps the state goes through torch.save /
    torch.load into a fresh instance on cloned parameters; three more steps of both on the same gradients give the same bits."""
    trio = Trio(kernel, "adam")
    trio.step(none=(4,))
    trio.steps(2)
    assert trio.counts() == [3.0, 3.0, 3.0, 3.0, 2.0]
    loaded = through_a_file(trio.fused.state_dict())
    resumed = FusedAdam(OC.groups_of([torch.nn.Parameter(p.detach().clone()) for p in flat(trio.fused)]), lr=1.0)
    resumed.load_state_dict(loaded)
    assert [g["lr"] for g in resumed.param_groups] == [1e-3, 3e-3]
    for _ in range(3):
        trio.step()
        OC.set_grads(resumed, [p.grad for p in flat(trio.fused)])
        kernel.opt = resumed
        resumed.step()
        for i, (p, q) in enumerate(zip(flat(trio.fused), flat(resumed))):
            a, b = trio.fused.state[p], resumed.state[q]
            assert bits_equal(p.detach(), q.detach()) and float(a["step"]) == float(b["step"]), i
            assert bits_equal(a["exp_avg"], b["exp_avg"]) and bits_equal(a["exp_avg_sq"], b["exp_avg_sq"]), i
    assert trio.counts(resumed) == [6.0, 6.0, 6.0, 6.0, 5.0]


def donor_state():
    """The state_dict of a torch.optim.Adam over the five shapes after three steps, position 4 with two."""
    donor = torch.optim.Adam(OC.groups_of(OC.five_params(CPU, seed=21)), foreach=False)
    for k in range(3):
        grads = OC.fresh_grads(flat(donor), 500 + k, CPU)
        if k == 0:
            grads[4] = None
        OC.set_grads(donor, grads)
        donor.step()
    return donor.state_dict()


def test_torch_adam_state_loaded_into_an_instance_that_has_stepped(kernel):
    sd = donor_state()
    trio, _ = life(kernel, "adam", lambda opt: opt.load_state_dict(copy.deepcopy(sd)), before=2)
    assert trio.counts() == [6.0, 6.0, 6.0, 6.0, 5.0]


@pytest.mark.parametrize("form", ("int", "float", "tensor0d"))
def test_loaded_step_entries_that_are_numbers_or_0d_tensors(kernel, form):
    sd = donor_state()
    for st in sd["state"].values():
        n = int(st["step"])
        st["step"] = {"int": n, "float": float(n), "tensor0d": torch.tensor(float(n))}[form]
    trio, _ = life(kernel, "adam", lambda opt: opt.load_state_dict(copy.deepcopy(sd)), before=1)
    assert trio.counts() == [6.0, 6.0, 6.0, 6.0, 5.0]
    for p in flat(trio.fused):
        step = trio.fused.state[p]["step"]
        assert isinstance(step, torch.Tensor) and step.dtype == torch.float32 and step.dim() == 0 and step.device.type == "cpu"


def test_state_dict_kept_while_training_goes_on(kernel):
    """What a ``state_dict()`` that is kept in memory shows of the steps taken after it: the same as torch.optim.Adam's."""
    trio = Trio(kernel, "adam")
    trio.steps(2)
    kept = trio.each(lambda opt: opt.state_dict())
    was = [(float(sd["state"][3]["step"]), sd["state"][3]["exp_avg"].clone()) for sd in kept]
    trio.steps(2)
    shared = [(float(sd["state"][3]["step"]) != step, not bits_equal(sd["state"][3]["exp_avg"], m)) for sd, (step, m) in zip(kept, was)]
    print("state_dict() kept over two steps, (step moved, exp_avg moved):", dict(zip(Trio.NAMES, shared)))
    assert shared[0] == shared[1] == shared[2]
    for sd, opt in zip(kept, trio.opts):                              # and a deep copy of it, as a checkpoint is, loads
        twin = type(opt)(OC.groups_of([torch.nn.Parameter(p.detach().clone()) for p in flat(opt)]))
        twin.load_state_dict(copy.deepcopy(sd))
        assert [float(twin.state[p]["step"]) for p in flat(twin)] == [float(sd["state"][i]["step"]) for i in range(5)]


# ---- copies of the optimiser ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ("deepcopy", "pickle"))
def test_copies_step_independently(kernel, how):
    duplicate = copy.deepcopy if how == "deepcopy" else lambda opt: pickle.loads(pickle.dumps(opt))
    trio = Trio(kernel, "adam")
    trio.step(none=(4,))
    trio.steps(2)
    other = Trio(kernel, "adam", opts=trio.each(duplicate))
    other.k = 50
    for a, b in zip(trio.opts, other.opts):
        assert type(a) is type(b) and all(p is not q and bits_equal(p.detach(), q.detach()) for p, q in zip(flat(a), flat(b)))
    assert other.fused._plans == {} and trio.fused._plans != {}
    mine = [trio.fused.state[p]["step"] for p in flat(trio.fused)]    # the tensors themselves, not their values
    bits = [p.detach().clone() for p in flat(trio.fused)]
    other.steps(2)                                                    # (gated and compared among the three copies)
    assert other.counts() == [5.0, 5.0, 5.0, 5.0, 4.0]
    assert [float(s) for s in mine] == [3.0, 3.0, 3.0, 3.0, 2.0] and trio.counts() == [3.0, 3.0, 3.0, 3.0, 2.0]
    assert all(bits_equal(p.detach(), was) for p, was in zip(flat(trio.fused), bits))
    theirs = [other.fused.state[p]["step"] for p in flat(other.fused)]
    trio.steps(3)
    assert trio.counts() == [6.0, 6.0, 6.0, 6.0, 5.0]
    assert [float(s) for s in theirs] == [5.0, 5.0, 5.0, 5.0, 4.0] and other.counts() == [5.0, 5.0, 5.0, 5.0, 4.0]
