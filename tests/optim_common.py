"""What tests/test_optim_host.py and tests/test_optim_gpu.py share: one Adam / SGD step restated in float64 with the error bounds of
DESIGN.md 7s, the seeded inputs those bounds were checked on, a float32 NumPy restatement of the kernel's arithmetic with three
deliberately wrong variants (so that the gate is shown to fail without a GPU), and the driver that records a scheduler's lr
sequence (tests/golden/make_scheduler_golden.py runs it on the reference's classes, the host test on this package's).

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
