"""The optimiser step's host side (no GPU): the argument checks of balf_adam_step / balf_sgd_step, which return before any launch;
the error bounds of tests/optim_common.py held against a float32 NumPy restatement of the kernel and against three wrong variants
(the gate of tests/test_optim_gpu.py can fail); and what balf_amd.utils.train_utils adds for the reference's train.py:
build_optimizer, build_scheduler, WarmRestart, LinearDecay (lr sequences equal to the reference's, tests/golden/schedulers.json)
and ckpt_state."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from balf_amd import _lib
from balf_amd.utils import train_utils
from tests import optim_common as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


# ---- argument checks: every call below is refused (or has nothing to do) on the host, before anything is launched -----------------
def ptrs(values):
    return (C.c_void_p * len(values))(*values)


def counts(values):
    return (C.c_int64 * len(values))(*values)


class Call:
    """A well-formed call on n fake device pointers (never dereferenced: every use below fails a check first, or skips all)."""

    def __init__(self, n=3):
        self.n = n
        self.p, self.g, self.m, self.v = (ptrs([base + 4096 * i for i in range(n)]) for base in (1 << 20, 2 << 20, 3 << 20, 4 << 20))
        self.numel = counts([16] * n)
        self.hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)

    def adam(self, lib, **kw):
        h = dict(self.hyper, **{k: kw.pop(k) for k in list(kw) if k in self.hyper})
        a = dict(n=self.n, p=self.p, g=self.g, m=self.m, v=self.v, numel=self.numel)
        a.update(kw)
        return lib.balf_adam_step(a["n"], a["p"], a["g"], a["m"], a["v"], a["numel"], h["lr"], h["beta1"], h["beta2"], h["eps"],
                                  h["weight_decay"], h["step"], None)

    def sgd(self, lib, lr=1e-3, **kw):
        a = dict(n=self.n, p=self.p, g=self.g, numel=self.numel)
        a.update(kw)
        return lib.balf_sgd_step(a["n"], a["p"], a["g"], a["numel"], lr, None)


def with_entry(arr, i, value):
    out = (C.c_void_p * len(arr))(*arr)
    out[i] = value
    return out


def test_chunk_elems(lib):
    c = lib.balf_optim_chunk_elems()
    assert c > 0 and c % 4 == 0


def test_adam_argument_checks(lib):
    c = Call()
    assert c.adam(lib, n=0) == ARG and c.adam(lib, n=-1) == ARG and c.adam(lib, n=65) == ARG
    for name in ("p", "g", "m", "v", "numel"):
        assert c.adam(lib, **{name: None}) == ARG, name                                     # a null array
    for name in ("p", "m", "v"):
        assert c.adam(lib, **{name: with_entry(getattr(c, name), 1, None)}) == ARG, name    # a null entry with numel > 0
    for name in ("p", "g", "m", "v"):
        for off in (1, 2, 3):
            assert c.adam(lib, **{name: with_entry(getattr(c, name), 2, getattr(c, name)[2] + off)}) == ARG, (name, off)
    assert c.adam(lib, numel=counts([16, -1, 16])) == ARG
    for name in ("lr", "eps", "weight_decay"):
        for bad in (-1e-3, -0.5, math.nan, math.inf, -math.inf):
            assert c.adam(lib, **{name: bad}) == ARG, (name, bad)
    for name in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, 1.5, math.nan, math.inf):
            assert c.adam(lib, **{name: bad}) == ARG, (name, bad)
    assert c.adam(lib, step=0) == ARG and c.adam(lib, step=-3) == ARG
    # an error is reported even when the offending tensor would be skipped
    assert c.adam(lib, g=ptrs([None] * 3), numel=counts([16, -1, 16])) == ARG
    assert c.adam(lib, g=ptrs([None] * 3), lr=-1.0) == ARG


def test_sgd_argument_checks(lib):
    c = Call()
    assert c.sgd(lib, n=0) == ARG and c.sgd(lib, n=65) == ARG
    for name in ("p", "g", "numel"):
        assert c.sgd(lib, **{name: None}) == ARG, name
    assert c.sgd(lib, p=with_entry(c.p, 0, None)) == ARG
    for name in ("p", "g"):
        assert c.sgd(lib, **{name: with_entry(getattr(c, name), 1, getattr(c, name)[1] + 2)}) == ARG, name
    assert c.sgd(lib, numel=counts([-5, 16, 16])) == ARG
    for bad in (-1e-3, math.nan, math.inf):
        assert c.sgd(lib, lr=bad) == ARG, bad


def test_too_many_chunks(lib):
    """2^31 chunks in all, one more than a launch has workgroups: refused as a shape, before the launch."""
    per = (1 << 31) // 64 * lib.balf_optim_chunk_elems()
    c = Call(64)
    assert c.adam(lib, numel=counts([per] * 64)) == SHAPE
    assert c.sgd(lib, numel=counts([per] * 64)) == SHAPE


def test_all_skipped_is_ok(lib):
    """No gradient anywhere, or no element anywhere: nothing to do, nothing launched, BALF_OK.  A null p / m / v entry is fine
    where numel is 0 (an empty tensor's data_ptr)."""
    c = Call()
    none = ptrs([None] * 3)
    assert c.adam(lib, g=none) == 0 and c.sgd(lib, g=none) == 0
    assert c.adam(lib, numel=counts([0] * 3)) == 0 and c.sgd(lib, numel=counts([0] * 3)) == 0
    assert c.adam(lib, p=none, m=none, v=none, numel=counts([0] * 3)) == 0
    assert c.adam(lib, g=with_entry(none, 1, c.g[1]), numel=counts([16, 0, 16])) == 0


# ---- the bounds, on the CPU -------------------------------------------------------------------------------------------------------
N_HOST = 200_000
HOST_CASES = [(wd, step) for wd in (0.0, 0.01) for step in (1, 2, 7, 1000)]


@pytest.fixture(scope="module")
def host_cases():
    """(wd, step) -> (inputs, float64 reference), computed once."""
    out = {}
    for i, (wd, step) in enumerate(HOST_CASES):
        x = OC.draw(N_HOST, i, wd)
        out[wd, step] = (x, OC.adam64(*x, step=step, wd=wd))
    return out


@pytest.mark.parametrize("wd,step", HOST_CASES)
def test_float32_restatement_is_within_the_bounds(host_cases, wd, step):
    x, ref = host_cases[wd, step]
    assert (x[1] == 0).sum() >= 100
    p1, m1, v1 = OC.adam32(*x, step=step, wd=wd)
    figs = OC.check_adam(f"numpy float32 wd={wd} step={step}", p1, m1, v1, ref)
    assert figs["p"] > 0.5                                                         # the bound is not loose: the last rounding alone reaches u |p'|


@pytest.mark.parametrize("mutant", OC.MUTANTS)
def test_wrong_variants_leave_the_bound(host_cases, mutant):
    """eps inside the square root, no bias correction, decoupled weight decay: each leaves the p' bound on a large share of the
    elements of every case in which it differs from Adam at all (decoupled decay needs wd != 0; the bias corrections are ~1 only
    at step 1000 for b1, never for b2)."""
    for (wd, step), (x, ref) in host_cases.items():
        if mutant == "decoupled_wd" and wd == 0:
            continue
        p1, _, _ = OC.adam32(*x, step=step, wd=wd, mutant=mutant)
        out = np.abs(p1.astype(np.float64) - ref["p"]) > ref["bp"]
        print(f"{mutant} wd={wd} step={step}: {out.mean():.3f} of the elements outside the p' bound")
        assert out.mean() > 0.25, (mutant, wd, step, out.mean())


def test_sgd_restatement_is_within_its_bound(host_cases):
    (p, g, _, _), _ = host_cases[0.0, 1]
    ref = OC.sgd64(p, g, 1e-2)
    got = p - np.float32(1e-2) * g
    assert OC.excess(got, ref["p"], ref["bp"]) <= 1.0
    assert OC.excess(p - np.float32(1.1e-2) * g, ref["p"], ref["bp"]) > 1.0


# ---- build_optimizer, build_scheduler, the schedulers, ckpt_state ------------------------------------------------------------------
def cpu_params():
    return [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]


def test_build_optimizer_on_cpu_parameters():
    adam = train_utils.build_optimizer(cpu_params(), {"name": "adam", "lr": 2e-3, "weight_decay": 1e-4})
    assert type(adam) is torch.optim.Adam
    assert adam.param_groups[0]["lr"] == 2e-3 and adam.param_groups[0]["weight_decay"] == 1e-4 and not adam.param_groups[0]["amsgrad"]
    sgd = train_utils.build_optimizer(iter(cpu_params()), {"name": "sgd", "lr": 0.1})          # a generator, as model.parameters()
    assert type(sgd) is torch.optim.SGD and sgd.param_groups[0]["lr"] == 0.1 and sgd.param_groups[0]["momentum"] == 0
    with pytest.raises(ValueError, match=r"^Optimizer \[rmsprop\] not recognized\.$"):
        train_utils.build_optimizer(cpu_params(), {"name": "rmsprop", "lr": 1e-3})


def test_build_scheduler():
    opt = torch.optim.SGD(cpu_params(), lr=1e-3)
    s = train_utils.build_scheduler(opt, 50, -1, {"name": "plateau", "patience": 3, "factor": 0.5, "min_lr": 1e-6})
    assert type(s) is torch.optim.lr_scheduler.ReduceLROnPlateau and s.patience == 3 and s.factor == 0.5 and s.mode == "min"
    assert s.min_lrs == [1e-6]
    s = train_utils.build_scheduler(opt, 50, -1, {"name": "sgdr"})
    assert type(s) is train_utils.WarmRestart and s.T_max == 30 and s.T_mult == 1 and s.eta_min == 0
    s = train_utils.build_scheduler(opt, 50, -1, {"name": "linear", "min_lr": 1e-5, "start_epoch": 7})
    assert type(s) is train_utils.LinearDecay and (s.max_epoch, s.start_epoch, s.min_lr) == (50, 7, 1e-5)
    s = train_utils.build_scheduler(opt, 50, 19, {"name": "linear", "min_lr": 1e-5, "start_epoch": 7})     # resumed: initial_lr is there
    assert s.last_epoch == 20
    with pytest.raises(ValueError, match=r"^Scheduler \[step\] not recognized\.$"):
        train_utils.build_scheduler(opt, 50, -1, {"name": "step"})


@pytest.mark.parametrize("name", sorted(OC.SCHEDULER_CASES))
def test_scheduler_lr_sequences_equal_the_reference(name):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "schedulers.json")))
    assert fx["meta"]["epochs"] == OC.EPOCHS == 70 and tuple(fx["meta"]["base_lrs"]) == OC.BASE_LRS
    assert fx["meta"]["cases"][name] == {"class": OC.SCHEDULER_CASES[name][0], "kwargs": OC.SCHEDULER_CASES[name][1]}
    got = OC.lr_sequence({"WarmRestart": train_utils.WarmRestart, "LinearDecay": train_utils.LinearDecay}, name)
    want = fx["lr"][name]
    assert len(got) == len(want) == 70
    assert got == want                                                             # equal as floats, both groups, every epoch
    assert len({row[0] for row in want}) > 20                                      # (a sequence, not a constant)


def test_ckpt_state():
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    s = train_utils.ckpt_state(model, opt, 4, 61.5)
    assert list(s) == ["epoch", "model_state", "optimizer_state", "repeatability"]
    assert s["epoch"] == 4 and s["repeatability"] == 61.5
    assert list(s["model_state"]) == ["weight", "bias"] and set(s["optimizer_state"]) == {"state", "param_groups"}
    assert train_utils.ckpt_state() == {"epoch": None, "model_state": None, "optimizer_state": None, "repeatability": 0.0}
