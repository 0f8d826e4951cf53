"""Shared by tests/test_head_train_host.py, tests/test_head_train_gpu.py, tests/golden/make_head_train_golden.py and
tools/bench_head_train.py: the fixture head_train.npz, the float64 restatement of the trainable tail (down4.conv2 -> ReLU ->
detector_head.dense -> BatchNorm2d with batch statistics) and of its backward as closed formulas, the same through float64
autograd, the float32 torch-op composition, the error measure of the gates, and the seeded case generator of the shape sweep."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import train_common as T
from tests.train_common import err                # noqa: F401  (H.err, as the tests and tools name it)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train.npz")
FIXTURE_CASES = ("model", "edges")
PARAMS = ("w2", "b2", "wd", "bd", "gamma", "beta")
GRADS = ("dw2", "db2", "dwd", "dbd", "dgamma", "dbeta", "dx2")
GATED = ("logits",) + GRADS + ("running_mean", "running_var")
TOL_FLOOR = 1.1e-6              # three chained fp32-MFMA GEMMs at <= 3.5e-7 * sum |a b| each (K <= 4096)
EPS, MOMENTUM = 1e-5, 0.1
KINK_MARGIN = 2e-5              # no pre-activation of a fixture case lies this close to the ReLU kink, except exact zeros


def fixture():
    return np.load(FIXTURE)


def pixel_shuffle8(p64):
    """[B,64,Hc,Wc] -> [B,8Hc,8Wc], channel dy * 8 + dx to pixel (8y + dy, 8x + dx) (tensor_op.pixel_shuffle, one output channel)."""
    b, _, hc, wc = p64.shape
    return p64.reshape(b, 8, 8, hc, wc).permute(0, 3, 1, 4, 2).reshape(b, 8 * hc, 8 * wc)


def restate64(x2, p, dlogits=None, stats=None, running=None, eps=EPS, momentum=MOMENTUM):
    """The equations of include/balf_hip.h in float64 on the CPU.  ``x2`` [B,Hc,Wc,256]; ``p``: dict of the six parameters
    (PARAMS); ``dlogits`` [B,65,Hc,Wc] or None; ``stats`` [2,65] (mean, variance) = eval mode; ``running`` (mean, var) to update.
    -> dict of float64 torch tensors: the outputs, the intermediates (h, a, z, xhat, r) and ``S``: name -> the scale of the
    error measure, the largest sum of absolute values of the terms of that output's last reduction."""
    b, hc, wc, _ = x2.shape
    n = b * hc * wc
    X = x2.reshape(n, 256).double()
    w2, b2, wd, bd, gamma, beta = (p[k].double() for k in PARAMS)
    h = X @ w2.T + b2
    a = h.clamp(min=0)
    z = a @ wd.T + bd
    if stats is None:
        mu, var = z.mean(0), z.var(0, unbiased=False)
    else:
        mu, var = stats[0].double(), stats[1].double()
    r = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mu) * r
    flat = gamma * xhat + beta

    def nchw(t):
        return t.reshape(b, hc, wc, 65).permute(0, 3, 1, 2).contiguous()

    out = {"h": h, "a": a, "z": z, "xhat": xhat, "r": r, "mean": mu, "var": var, "logits": nchw(flat),
           "prob": pixel_shuffle8(torch.softmax(nchw(flat), dim=1)[:, :64])}
    S = {"logits": float((((a.abs() @ wd.abs().T) + bd.abs()) * r * gamma.abs() + beta.abs()).max())}
    if running is not None and stats is None:
        rm, rv = running[0].double(), running[1].double()
        unbiased = var * n / (n - 1)
        out["running_mean"], out["running_var"] = (1 - momentum) * rm + momentum * mu, (1 - momentum) * rv + momentum * unbiased
        S["running_mean"] = float(((1 - momentum) * rm.abs() + momentum * mu.abs()).max())
        S["running_var"] = float(((1 - momentum) * rv.abs() + momentum * unbiased.abs()).max())
    if dlogits is not None:
        g = dlogits.double().permute(0, 2, 3, 1).reshape(n, 65)
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
        dz = gamma * r * (g - dbeta / n - xhat * dgamma / n)
        da = dz @ wd
        dh = da * (h > 0)
        out.update(dbeta=dbeta, dgamma=dgamma, dz=dz, dwd=dz.T @ a, dbd=dz.sum(0), dh=dh, dw2=dh.T @ X, db2=dh.sum(0),
                   dx2=(dh @ w2).reshape(b, hc, wc, 256))
        S.update(dbeta=float(g.abs().sum(0).max()), dgamma=float((g * xhat).abs().sum(0).max()),
                 dwd=float((dz.abs().T @ a.abs()).max()), dbd=float(dz.abs().sum(0).max()),
                 dw2=float((dh.abs().T @ X.abs()).max()), db2=float(dh.abs().sum(0).max()),
                 dx2=float((dh.abs() @ w2.abs()).max()))
    out["S"] = S
    return out


def autograd64(x2, p, dlogits, eps=EPS):
    """The same gradients from float64 autograd over torch's own linear / relu / batch_norm -> dict GRADS."""
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    x = x2.double().clone().requires_grad_()
    z = F.linear(F.relu(F.linear(x, leaves["w2"], leaves["b2"])), leaves["wd"], leaves["bd"]).permute(0, 3, 1, 2)
    logits = F.batch_norm(z, None, None, leaves["gamma"], leaves["beta"], training=True, momentum=0.0, eps=eps)
    (logits * dlogits.double()).sum().backward()
    out = {"d" + k: leaves[k].grad for k in PARAMS}
    out["dx2"] = x.grad
    return out


def compose_f32(x2, p, dlogits=None, running=None, eps=EPS, momentum=MOMENTUM):
    """The float32 torch-op composition on the tensors' device (what tools/bench_head_train.py times): F.linear, F.relu,
    F.linear, F.batch_norm(training=True) and, with ``dlogits``, their autograd -> (logits, dict GRADS or None)."""
    leaves = {k: p[k].detach().clone().requires_grad_(dlogits is not None) for k in PARAMS}
    x = x2.detach().clone().requires_grad_(dlogits is not None)
    z = F.linear(F.relu(F.linear(x, leaves["w2"], leaves["b2"])), leaves["wd"], leaves["bd"]).permute(0, 3, 1, 2)
    rm, rv = running if running is not None else (None, None)
    logits = F.batch_norm(z, rm, rv, leaves["gamma"], leaves["beta"], training=True, momentum=momentum, eps=eps)
    if dlogits is None:
        return logits, None
    logits.backward(dlogits)
    grads = {"d" + k: leaves[k].grad for k in PARAMS}
    grads["dx2"] = x.grad
    return logits.detach(), grads


def kink_distance(h):
    """The smallest |h| among the pre-activations that are not exactly zero."""
    nz = h[h != 0]
    return float(nz.abs().min()) if nz.numel() else float("inf")


def sweep_params(seed, exact_z=False):
    """Seeded parameters for the shape sweep.  w2 holds multiples of 1/16 and b2 odd multiples of 1/256 (see sweep_case); with
    ``exact_z`` wd holds multiples of 1/4 in [-1/2, 1/2] and bd multiples of 1/4 as well."""
    g = torch.Generator().manual_seed(seed)
    p = {"w2": torch.randint(-8, 9, (256, 256), generator=g).float() / 16,
         "b2": (2 * torch.randint(-64, 64, (256,), generator=g) + 1).float() / 256,
         "wd": torch.randn((65, 256), generator=g) / 16, "bd": torch.randn((65,), generator=g) * 0.5,
         "gamma": 1 + 0.5 * torch.randn((65,), generator=g), "beta": 0.3 * torch.randn((65,), generator=g)}
    if exact_z:
        p["wd"] = torch.randint(-2, 3, (65, 256), generator=g).float() / 4
        p["bd"] = torch.randint(-8, 9, (65,), generator=g).float() / 4
    return p


def sweep_case(shape, seed, device=None):
    """Seeded inputs for a shape without a fixture -> (x2 [B,Hc,Wc,256], params, dlogits [B,65,Hc,Wc], (running_mean,
    running_var)), float32 on the CPU.

    x2 holds multiples of 1/8 in [-1, 1], w2 multiples of 1/16 in [-1/2, 1/2] and b2 odd multiples of 1/256: every product is a
    multiple of 1/128, a sum of 256 of them plus b2 is an odd multiple of 1/256 below 2^8 -- exact in float32 in any order and
    never closer than 1/256 to the ReLU kink.  So the mask [h > 0] of a float32 implementation cannot differ from the float64
    restatement's by a rounding of h (a flipped element would be an error of a whole term, at any tolerance), while a, z and
    everything after them are general float32 values.  The float32 rounding of the first product itself is covered by the
    fixture cases, whose inputs are general and whose distance from the kink is recorded.

    The two shapes with N = 2 go one step further.  With two samples dz is gamma r (g1 - g2) / 2 * eps / (var + eps) with var =
    (z1 - z2)^2 / 4: a relative perturbation of z comes out multiplied by 3 |z| / |z1 - z2|, and the channels with the smallest
    |z1 - z2| carry the largest dz.  A float32 rounding of z (1e-7 of sum |a wd|) then shows as 1e-5 .. 1e-3 in every gradient,
    in ANY float32 implementation: torch's own float32 composition on the CPU measured dw2 2.3e-5 at (1,1,2) and 1.0e-3 at
    (2,1,1) on general wd, against a gate of 1.1e-6.  So for N = 2 wd and bd are quantised too (multiples of 1/4): z = a wd^T +
    bd is a sum of multiples of 1/1024 below 2^11, exact in float32, and what remains is what these two shapes are in the sweep
    for: the two-sample statistics, the cancellation in dz, the batch stride at one pixel per image and the smallest grids.

    ``device``: where the case is moved to after it was drawn, on the CPU generator either way, so that restate64 and
    compose_f32 run there (a shape of tens of thousands of pixels)."""
    b, hc, wc = shape
    g = torch.Generator().manual_seed(1000 + seed)
    x2 = torch.randint(-8, 9, (b, hc, wc, 256), generator=g).float() / 8
    dlogits = torch.randn((b, 65, hc, wc), generator=g) / (b * hc * wc)
    running = (torch.randn((65,), generator=g), 0.5 + torch.rand((65,), generator=g))
    return T.to_device((x2, sweep_params(seed, exact_z=b * hc * wc == 2), dlogits, running), device)


# ---- the fixture cases' inputs that need not be stored: seeded, and the checkpoint's own tail -----------------------------------
_SD_NAMES = {"w2": "down4.conv2.weight", "b2": "down4.conv2.bias", "wd": "detector_head.dense.weight",
             "bd": "detector_head.dense.bias", "gamma": "detector_head.norm.weight", "beta": "detector_head.norm.bias"}


def params_of(sd):
    """The tail's six parameters and its running statistics out of a detector state dict -> (dict PARAMS, (mean, var))."""
    return ({k: sd[n].detach().clone().float() for k, n in _SD_NAMES.items()},
            (sd["detector_head.norm.running_mean"].detach().clone().float(),
             sd["detector_head.norm.running_var"].detach().clone().float()))


def model_inputs():
    """Case ``model`` without its stored x2: the tail of synth.synthetic_state_dict(0), the seeded image that the recorder feeds
    to the reference's network, and the seeded dlogits -> (image [2,3,64,64], params, dlogits [2,65,8,8], running)."""
    from balf_amd.utils import synth
    p, running = params_of(synth.synthetic_state_dict(0))
    rng = np.random.Generator(np.random.PCG64([2024, 1]))
    image = torch.from_numpy(rng.random((2, 3, 64, 64)).astype(np.float32))
    dlogits = torch.from_numpy((rng.standard_normal((2, 65, 8, 8)) / 128).astype(np.float32))
    return image, p, dlogits, running


EDGES_SHAPE = (3, 3, 5)
EDGES_ZERO_ROWS = ((0, 0, 0), (2, 1, 3))        # all-zero feature rows: with b2 = 0 on channels 0..7, h == 0 exactly there
EDGES_GAMMA0, EDGES_SHIFTED = 5, 9              # the channel with gamma = 0; the channel with bd + 100 (mean^2 >> var)


def edges_inputs():
    """Case ``edges`` -> (x2 [3,3,5,256], params, dlogits [3,65,3,5], running): seeded features x 8 on the same checkpoint's
    tail, with the three edges named above."""
    from balf_amd.utils import synth
    p, running = params_of(synth.synthetic_state_dict(0))
    rng = np.random.Generator(np.random.PCG64([2024, 2]))
    b, hc, wc = EDGES_SHAPE
    x2 = torch.from_numpy((8 * rng.standard_normal((b, hc, wc, 256))).astype(np.float32))
    for at in EDGES_ZERO_ROWS:
        x2[at] = 0.0
    p["b2"][:8] = 0.0
    p["gamma"][EDGES_GAMMA0] = 0.0
    p["bd"][EDGES_SHIFTED] += 100.0
    dlogits = torch.from_numpy((rng.standard_normal((b, 65, hc, wc)) / (b * hc * wc)).astype(np.float32))
    return x2, p, dlogits, running


def inputs_digest(*tensors):
    """train_common.inputs_digest, a dict of parameters in PARAMS order."""
    return T.inputs_digest(*tensors, keys=lambda d: PARAMS)


def regenerated_inputs_digest(name):
    """The digest of everything of case ``name`` that the fixture does not store."""
    if name == "model":
        return inputs_digest(*model_inputs())
    return inputs_digest(*edges_inputs())


def fixture_case(fx, name):
    """-> (x2, params, dlogits, running) of a fixture case, float32 on the CPU."""
    if name == "model":
        _, p, dlogits, running = model_inputs()
        return torch.from_numpy(fx["model.x2"]), p, dlogits, running
    return edges_inputs()


def train64(chunk, p, running, presentations, lr=1e-3, eps=EPS):
    """The float64 restatement of ``train_utils.train_head`` on the CPU: ``chunk`` a list of (feat_src, feat_dst, heat_src,
    heat_dst) CPU tensors, presented ``presentations`` times to torch.optim.Adam over float64 copies of the six parameters, the
    loss being detector_loss (tests/detector_loss_common.py: restate64, no noise) of both sides -> (the per-presentation mean
    losses, the trained parameters, the running statistics, updated as BatchNorm does)."""
    from tests import detector_loss_common as D
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    rm, rv = running[0].double().clone(), running[1].double().clone()
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    means = []
    for _ in range(presentations):
        losses = []
        for feat_src, feat_dst, heat_src, heat_dst in chunk:
            opt.zero_grad()
            total = 0.0
            for feat, heat in ((feat_src, heat_src), (feat_dst, heat_dst)):
                z = F.linear(F.relu(F.linear(feat.double(), leaves["w2"], leaves["b2"])), leaves["wd"], leaves["bd"]).permute(0, 3, 1, 2)
                logits = F.batch_norm(z, rm, rv, leaves["gamma"], leaves["beta"], training=True, momentum=MOMENTUM, eps=eps)
                r = D.restate64(logits.detach(), heat.float(), None, None)
                logits.backward(torch.from_numpy(r["grad"]))
                total += float(r["loss"])
            opt.step()
            losses.append(total)
        means.append(float(np.mean(losses)))
    return means, {k: v.detach() for k, v in leaves.items()}, (rm, rv)


def eval_loss64(chunk, p, running):
    """The mean over ``chunk`` of detector_loss(src) + detector_loss(dst) with the head in eval mode (running statistics), in
    float64: what ``train_utils.check_val_anchor_loss`` measures on a model that holds these parameters."""
    from tests import detector_loss_common as D
    total = []
    for feat_src, feat_dst, heat_src, heat_dst in chunk:
        total.append(sum(float(D.restate64(restate64(f, p, stats=torch.stack(running))["logits"], h.float(), None, None)["loss"])
                         for f, h in ((feat_src, heat_src), (feat_dst, heat_dst))))
    return float(np.mean(total))
