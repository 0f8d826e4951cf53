"""What tests/test_optim_host.py, tests/test_optim_gpu.py and the two tests/test_optim_life_*.py share: one Adam / SGD step restated
in float64 with the error bounds of DESIGN.md 7s, the seeded inputs those bounds were checked on, a float32 NumPy restatement of the
kernel's arithmetic with three deliberately wrong variants (so that the gate is shown to fail without a GPU), the driver that
records a scheduler's lr sequence (tests/golden/make_scheduler_golden.py runs it on the reference's classes, the host test on this
package's), and what drives an optimiser object step by step under those bounds on a device given by the caller (five_params ..
gate_step).

THE BOUNDS count roundings; u = 2^-24.  From the float32 inputs, in float64:
    G = |g| + wd |p|      A = b1 |m| + (1 - b1) G      D = sqrt(v') / sqrt(bc2) + eps      U = (lr / bc1) |m'| / D
    |m'_32 - m'| <= 4 u A
    |v'_32 - v'| <= 6 u (b2 v + (1 - b2) G^2)
    |p'_32 - p'| <= u |p'| + 16 u [ (lr / bc1) A / D + U sqrt((1 - b2) / bc2) G / D ]
The second term of the last bracket carries the rounding error of g' = g + wd p into the denominator through v': where g ~ -wd p
the sum cancels, and without that term the bound is exceeded by orders of magnitude by any float32 Adam.
SGD: |p'_32 - p'| <= u |p'| + 2 u lr |g|."""
import numpy as np
import torch

U = 2.0 ** -24
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def draw(n, seed, wd):
    """-> float32 (p, g, m, v) of n elements: |p| over 1e-4..10, |g| and |m| over 1e-8..10, v over 1e-16..100, log-uniform, signs
    at random; min(100, n // 4) elements with a zero gradient and min(1000, n // 4) with g = -wd p (1 +- 1e-6), the cancelling
    ones (zero gradients too when wd = 0)."""
    rng = np.random.default_rng([20240, seed, n])
    sign = lambda: rng.choice([-1.0, 1.0], n)                      # noqa: E731
    p = (sign() * _log_uniform(rng, 1e-4, 10.0, n)).astype(np.float32)
    g = sign() * _log_uniform(rng, 1e-8, 10.0, n)
    m = (sign() * _log_uniform(rng, 1e-8, 10.0, n)).astype(np.float32)
    v = _log_uniform(rng, 1e-16, 100.0, n).astype(np.float32)
    where = rng.permutation(n)
    nz, nc = min(100, n // 4), min(1000, n // 4)
    g[where[:nz]] = 0.0
    c = where[nz:nz + nc]
    g[c] = -wd * p[c].astype(np.float64) * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, c.size))
    return p, g.astype(np.float32), m, v


# ---- one step in float64, with its bounds -------------------------------------------------------------------------------------------
def adam64(p, g, m, v, step, wd, lr=LR, b1=BETA1, b2=BETA2, eps=EPS):
    """float32 arrays -> dict of float64 arrays: p, m, v after the step and the bounds bp, bm, bv."""
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        gp = g + wd * p
        m1 = b1 * m + (1.0 - b1) * gp
        v1 = b2 * v + (1.0 - b2) * gp * gp
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        d = np.sqrt(v1) / np.sqrt(bc2) + eps
        p1 = p - (lr / bc1) * m1 / d
        big_g = np.abs(g) + wd * np.abs(p)
        a = b1 * np.abs(m) + (1.0 - b1) * big_g
        u_ = (lr / bc1) * np.abs(m1) / d
        bm = 4.0 * U * a
        bv = 6.0 * U * (b2 * v + (1.0 - b2) * big_g * big_g)
        bp = U * np.abs(p1) + 16.0 * U * ((lr / bc1) * a / d + u_ * np.sqrt((1.0 - b2) / bc2) * big_g / d)
    return {"p": p1, "m": m1, "v": v1, "bp": bp, "bm": bm, "bv": bv}


def sgd64(p, g, lr):
    p, g = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g))
    p1 = p - lr * g
    return {"p": p1, "bp": U * np.abs(p1) + 2.0 * U * lr * np.abs(g)}


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def excess(got, want, bound):
    """-> max over the elements of |got - want| / bound (0 / 0 counts as 0): at most 1 when every element is within its bound."""
    err = np.abs(_host(got).astype(np.float64).reshape(-1) - want.reshape(-1))
    b = bound.reshape(-1)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / b)
    return float(r.max()) if r.size else 0.0


def check_adam(what, got_p, got_m, got_v, ref, keep=None):
    """Every element (``keep``: a boolean mask of those looked at) of the three results is within its bound; the peaks are printed
    before anything is asserted."""
    sel = slice(None) if keep is None else keep
    figs = {k: excess(_host(t).reshape(-1)[sel], ref[k].reshape(-1)[sel], ref["b" + k].reshape(-1)[sel])
            for k, t in (("p", got_p), ("m", got_m), ("v", got_v))}
    print(what, " ".join(f"{k}' at {e:.3f} of its bound" for k, e in figs.items()))
    for k, e in figs.items():
        assert e <= 1.0, (what, k, e)
    return figs


# ---- the kernel's arithmetic in float32 NumPy, and three wrong variants ----------------------------------------------------------------
MUTANTS = ("eps_in_sqrt", "no_bias_correction", "decoupled_wd")


def _fma(a, b, c):
    """fl32(a b + c) through float64: the product of two float32 is exact there, the sum is rounded to 53 bits and then to 24 (a
    double rounding, which differs from the fused operation in rare half-way cases by one float32 ulp's worth of 2^-29)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def adam32(p, g, m, v, step, wd, lr=LR, b1=BETA1, b2=BETA2, eps=EPS, mutant=None):
    """balf_adam_step's operations in its order (csrc/optim.hip: adam_elem) -> float32 (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if mutant == "no_bias_correction":
        bc1 = bc2 = 1.0
    step_size, sqrt_bc2 = f(lr / bc1), f(np.sqrt(bc2))
    with np.errstate(all="ignore"):
        if mutant == "decoupled_wd":
            p = p - f(lr * wd) * p
            gp = g
        else:
            gp = _fma(f(wd), p, g) if wd != 0 else g
        m1 = _fma(f(1.0 - b1), gp, f(b1) * m)
        v1 = _fma(f(1.0 - b2), gp * gp, f(b2) * v)
        if mutant == "eps_in_sqrt":
            den = np.sqrt(v1 / (sqrt_bc2 * sqrt_bc2) + f(eps))
        else:
            den = np.sqrt(v1) / sqrt_bc2 + f(eps)
        p1 = p - (step_size * m1) / den
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


# ---- lr sequences of the schedulers ---------------------------------------------------------------------------------------------------
EPOCHS = 70
BASE_LRS = (1e-3, 5e-4)                      # two parameter groups
# name -> (class name, constructor keywords); "last_epoch" != -1 is a resumed run (the groups carry initial_lr, as a loaded one's do)
SCHEDULER_CASES = {
    "warm_default": ("WarmRestart", {}),                                                      # T_max 30: restarts at 30 and 60
    "warm_mult": ("WarmRestart", {"T_max": 20, "T_mult": 2, "eta_min": 1e-5}),                # restarts at 20 and 60
    "warm_resumed": ("WarmRestart", {"T_max": 25, "eta_min": 1e-6, "last_epoch": 12}),        # restarts at 25 and 50 of its count
    "linear_default": ("LinearDecay", {"max_epoch": EPOCHS}),
    "linear_start_min": ("LinearDecay", {"max_epoch": EPOCHS, "start_epoch": 10, "min_lr": 1e-5}),
    "linear_resumed": ("LinearDecay", {"max_epoch": EPOCHS, "start_epoch": 10, "min_lr": 1e-5, "last_epoch": 24}),
    "linear_resumed_early": ("LinearDecay", {"max_epoch": 100, "start_epoch": 30, "min_lr": 2e-4, "last_epoch": 4}),
}


def lr_sequence(classes, name):
    """The lr of both groups at each of EPOCHS epochs (read, optimizer.step(), scheduler.step()) -> [EPOCHS][2] floats.
    ``classes``: mapping class name -> scheduler class."""
    cls, kw = SCHEDULER_CASES[name]
    params = [torch.nn.Parameter(torch.zeros(2)) for _ in BASE_LRS]
    opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)], lr=1.0)
    if kw.get("last_epoch", -1) != -1:
        for grp in opt.param_groups:
            grp["initial_lr"] = grp["lr"]
    sched = classes[cls](opt, **kw)
    seq = []
    for _ in range(EPOCHS):
        seq.append([float(grp["lr"]) for grp in opt.param_groups])
        opt.step()
        sched.step()
    return seq


# ---- an optimiser object, step by step, on the device the caller names -------------------------------------------------------------------
CHUNK = 2048                                 # balf_optim_chunk_elems(), for the callers that run without the library


def five_params(device, seed=11, chunk=CHUNK):
    g = torch.Generator().manual_seed(seed)
    shapes = ((1,), (65,), (256, 65), (chunk + 1,), (3,))
    return [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(device)) for s in shapes]


def groups_of(params):
    return [{"params": params[:3], "lr": 1e-3, "weight_decay": 0.0}, {"params": params[3:], "lr": 3e-3, "weight_decay": 0.01}]


def fresh_grads(params, seed, device):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(p.shape, generator=g) * float(10.0 ** torch.empty(1).uniform_(-3, 0, generator=g))).to(device) for p in params]


def snapshot(opt):
    """(p, m, v, steps done) per parameter from the optimiser's own float32 state (zeros before the first step)."""
    out = []
    for grp in opt.param_groups:
        for p in grp["params"]:
            st = opt.state.get(p, {})
            zeros = np.zeros(p.numel(), np.float32)
            out.append((p.detach().cpu().numpy().reshape(-1).copy(),
                        st["exp_avg"].cpu().numpy().reshape(-1).copy() if "exp_avg" in st else zeros,
                        st["exp_avg_sq"].cpu().numpy().reshape(-1).copy() if "exp_avg_sq" in st else zeros,
                        int(st["step"]) if "step" in st else 0))
    return out


def gate_step(what, opt, before, grads):
    """Every tensor of ``opt`` after a step is within the one-step bounds of the float64 step from ``before``.  (The state is read
    with ``get``: looking must not add an entry to the optimiser's state, whose length the fused classes watch.)"""
    i = 0
    for grp in opt.param_groups:
        for p in grp["params"]:
            p0, m0, v0, done = before[i]
            g = grads[i]
            st = opt.state.get(p, {})
            if g is None:
                assert bits_equal(p.detach().reshape(-1), torch.from_numpy(p0).to(p.device)) and int(st.get("step", 0)) == done, (what, i)
            else:
                assert int(st["step"]) == done + 1 and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
                ref = adam64(p0, g.cpu().numpy().reshape(-1), m0, v0, step=done + 1, wd=grp["weight_decay"], lr=grp["lr"],
                             b1=grp["betas"][0], b2=grp["betas"][1], eps=grp["eps"])
                check_adam(f"{what} tensor {i}", p.detach(), st["exp_avg"], st["exp_avg_sq"], ref)
            i += 1


def gate_sgd_step(what, opt, before, grads):
    """The same for ``p -= lr * g``: every parameter within the SGD bound of the float64 step from ``before``, or its bits kept."""
    i = 0
    for grp in opt.param_groups:
        for p in grp["params"]:
            p0, g = before[i][0], grads[i]
            if g is None:
                assert bits_equal(p.detach().reshape(-1), torch.from_numpy(p0).to(p.device)), (what, i)
            else:
                ref = sgd64(p0, g.cpu().numpy().reshape(-1), grp["lr"])
                assert excess(p.detach(), ref["p"], ref["bp"]) <= 1.0, (what, i)
            i += 1


def set_grads(opt, grads):
    i = 0
    for grp in opt.param_groups:
        for p in grp["params"]:
            p.grad = None if grads[i] is None else grads[i].clone()
            i += 1


# ---- the fused classes against two oracles, on the device the caller names ----------------------------------------------------------------
def flat(opt):
    return [p for grp in opt.param_groups for p in grp["params"]]


def new_param(shape, seed, device):
    return torch.nn.Parameter((0.1 * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(device))


def five_groups(kind, device, chunk=CHUNK):
    """-> a function that makes the two groups of ``groups_of`` on fresh, equal parameters (one of them of c + 1 elements)."""
    def make():
        params = five_params(device, chunk=chunk)
        assert params[3].numel() == chunk + 1
        if kind == "adam":
            return groups_of(params)
        return [{"params": params[:3], "lr": 1e-2}, {"params": params[3:], "lr": 3e-2}]
    return make


def seventy(kind, device, chunk=CHUNK):
    """-> a function that makes ONE group of 70 parameters of 1 .. 40 elements, two of them of c + 1: two launches, 64 + 6."""
    def make():
        sizes = [chunk + 1 if i in (5, 66) else i * 7 % 40 + 1 for i in range(70)]
        grp = {"params": [new_param((n,), 100 + i, device) for i, n in enumerate(sizes)], "lr": 1e-3}
        return [dict(grp, weight_decay=0.01) if kind == "adam" else grp]
    return make


class Trio:
    """The instance under test (``fused``), its plan-free twin (``free``) and torch's optimiser (``torch``) on equal tensors, stepped
    together and judged after every step:
    (a) the twin, whose ``_plans`` is emptied before every ``step()`` -- no cache, so nothing stale -- has the same bits in every
        parameter and moment and the same step counts;
    (b) ``torch.optim.Adam(foreach=False)`` / ``torch.optim.SGD`` under the same mutation passes the one-step float64 gate above (so
        do the fused instances), has the same step counts and the same parameters with state, and its parameters agree with the
        fused ones within rtol 1e-5 / atol 1e-7: both are float32 Adam, one step differs by ~1e-6 of an update of at most 3e-3,
        which is ~3e-9 per step over the at most 70 steps taken by any caller.
    ``kernel``: an object whose ``opt`` is set to the optimiser about to step and whose ``calls`` collects the sizes of its launches."""
    NAMES = ("fused", "plan-free", "torch")

    def __init__(self, kernel, kind, device, make=None, opts=None):
        from balf_amd.optim import FusedAdam, FusedSGD
        self.kernel, self.kind, self.device, self.k = kernel, kind, device, 0
        make = make or five_groups(kind, device)
        if opts is None:
            cls, theirs = (FusedAdam, torch.optim.Adam) if kind == "adam" else (FusedSGD, torch.optim.SGD)
            opts = (cls(make()), cls(make()), theirs(make(), foreach=False))
        self.opts = tuple(opts)
        self.fused, self.free, self.torch = self.opts
        self.calls = {}

    def each(self, f):
        return [f(opt) for opt in self.opts]

    def step(self, none=()):
        """One step of all three on the same gradients (``none``: the flat positions without one), gated and compared."""
        self.k += 1
        grads = fresh_grads(flat(self.fused), 1000 + self.k, self.device)
        for i in none:
            grads[i] = None
        gate = gate_step if self.kind == "adam" else gate_sgd_step
        for name, opt in zip(self.NAMES, self.opts):
            before = snapshot(opt)
            set_grads(opt, grads)
            if opt is self.free:
                opt._plans = {}
            self.kernel.opt, self.kernel.calls = opt, []
            opt.step()
            self.calls[name] = self.kernel.calls
            gate(f"{name} step {self.k}", opt, before, grads)
        self.compare()

    def steps(self, n, none=()):
        for _ in range(n):
            self.step(none)

    def counts(self, opt=None):
        opt = opt or self.fused
        return [float(opt.state[p]["step"]) if opt.state.get(p) else None for p in flat(opt)]

    def compare(self):
        a, b, t = (flat(opt) for opt in self.opts)
        assert len(a) == len(b) == len(t)
        for i, (p, q, r) in enumerate(zip(a, b, t)):
            assert bits_equal(p.detach(), q.detach()), (i, "the plan-free twin's parameter differs")
            sp, sq, sr = self.fused.state.get(p, {}), self.free.state.get(q, {}), self.torch.state.get(r, {})
            assert set(sp) == set(sq) == set(sr), (i, set(sp), set(sq), set(sr))
            for key in sp:
                if key == "step":
                    assert float(sp[key]) == float(sq[key]) == float(sr[key]), (i, float(sp[key]), float(sq[key]), float(sr[key]))
                else:
                    assert sp[key].shape == p.shape and bits_equal(sp[key], sq[key]), (i, key)
            torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-5, atol=1e-7, msg=lambda m: f"parameter {i} against torch: {m}")
        entries = [sum(1 for v in opt.state.values() if v) for opt in self.opts]      # (those of parameters that left a list too)
        assert entries[0] == entries[1] == entries[2], entries


def life(kernel, kind, device, mutate, before=3, after=3, none_before=(), none_after=()):
    """``before`` steps, ``mutate(opt)`` on each of the three, ``after`` steps -> (the trio, what mutate returned per optimiser)."""
    trio = Trio(kernel, kind, device)
    trio.steps(before, none_before)
    out = trio.each(mutate)
    trio.steps(after, none_after)
    return trio, out
