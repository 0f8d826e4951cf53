"""Shared by tests/test_rcab_train_host.py, tests/test_rcab_train_gpu.py, tests/golden/make_rcab_train_golden.py and
tools/bench_tail_train.py, and by the stage-3 tests through tests/stage3_train_common.py: the fixture rcab_train.npz, the float64
restatement of the channel-attention block (LayerNorm -> conv1 -> LeakyReLU(0.2) -> conv2 -> squeeze-excite scale, x2 = t * s + r)
and of its backward as closed formulas, the same through float64 autograd, the float32 torch-op composition, the error measure of
the gates, and the seeded case generators.  All of it at a width C: the last dimension of the input where there is one, ``c``
(256, stage 4's, unless stated) in the generators; the squeeze-excite has C / 4 units."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import head_train_common as H
from tests import train_common as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcab_train.npz")
FIXTURE_CASES = ("model", "edges")
PARAMS = ("ln_g", "ln_b", "wc1", "bc1", "wc2", "bc2", "ws0", "bs0", "ws2", "bs2")        # = balf_amd.ops.RCAB_PARAMS
GRADS = tuple("d" + k for k in PARAMS) + ("dy",)
GATED = ("x2",) + GRADS                     # the twelve outputs
TOL_FLOOR = H.TOL_FLOOR                     # up to three chained fp32 GEMMs; no output here chains more (dn: dt wc2, dh wc1 after t)
LN_EPS = 1e-5
SLOPE = 0.2
# No pre-activation of a fixture case lies this close to a kink (of the LeakyReLU: h; of the SE ReLU: m ws0^T + bs0), except
# exact zeros: above the largest movement of h under a float32 evaluation, which is 3.3e-6 on the sweep's inputs and 2.8e-6 on
# case ``model`` with torch's own float32 ops on the CPU (|h| <= 12 there).  Case ``model`` is a given -- the checkpoint and
# the image are seeded -- and its closest h lies at 4.9e-6, where torch's float32 moved it by 1.5e-8.
KINK_MARGIN = 4e-6
SWEEP_MARGIN = 1e-3                         # the sweep's inputs keep every h and every SE pre-activation this far from 0
_SD_BLOCK = "residual_channel_attention_block."
SD_NAMES = dict(zip(PARAMS, ("norm.weight", "norm.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                              "calayer.excite.0.weight", "calayer.excite.0.bias", "calayer.excite.2.weight",
                              "calayer.excite.2.bias")))
err, inputs_digest = T.err, T.inputs_digest


def fixture():
    return np.load(FIXTURE)


def restate64(y, r, p, g=None):
    """The equations of include/balf_hip.h in float64 on the CPU.  ``y``, ``r`` [B,Hc,Wc,C]; ``p``: dict PARAMS; ``g`` = dx2 or
    None.  -> dict of float64 tensors: x2, the intermediates, the eleven gradients, and ``S``: name -> the scale of the error
    measure, the largest sum of absolute values of the terms of that output's last reduction (for x2 and dy the terms that
    follow the reduction are carried along: t * s + r, and rstd times the three terms of the LayerNorm's backward)."""
    b, hc, wc, c = y.shape
    hw, n_pix = hc * wc, b * hc * wc
    Y, R = y.reshape(n_pix, c).double(), r.reshape(n_pix, c).double()
    ln_g, ln_b, wc1, bc1, wc2, bc2, ws0, bs0, ws2, bs2 = (p[k].double() for k in PARAMS)
    mean = Y.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((Y - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    xhat = (Y - mean) * rstd
    n = xhat * ln_g + ln_b
    h = n @ wc1.T + bc1
    a = torch.where(h > 0, h, SLOPE * h)
    t = a @ wc2.T + bc2
    m = t.reshape(b, hw, c).mean(1)
    pre = m @ ws0.T + bs0
    e = pre.clamp(min=0)
    s = torch.sigmoid(e @ ws2.T + bs2)
    sp = s.repeat_interleave(hw, dim=0)                     # [N,C]
    out = {"xhat": xhat, "rstd": rstd, "n": n, "h": h, "a": a, "t": t, "m": m, "se_pre": pre, "e": e, "s": s,
           "x2": (t * sp + R).reshape(y.shape)}
    S = {"x2": float((((a.abs() @ wc2.abs().T) + bc2.abs()) * sp + R.abs()).max())}
    if g is not None:
        G = g.reshape(n_pix, c).double()
        ds = (G * t).reshape(b, hw, c).sum(1)
        dq = ds * s * (1 - s)
        de = (dq @ ws2) * (pre > 0)
        dm = de @ ws0
        dt = G * sp + (dm / hw).repeat_interleave(hw, dim=0)
        da = dt @ wc2
        slope = torch.where(h > 0, torch.ones_like(h), torch.full_like(h, SLOPE))
        dh = da * slope
        dn = dh @ wc1
        u = dn * ln_g
        dy = G + rstd * (u - u.mean(1, keepdim=True) - xhat * (u * xhat).mean(1, keepdim=True))
        out.update(ds=ds, dq=dq, de=de, dm=dm, dt=dt, dh=dh, dn=dn, dln_g=(dn * xhat).sum(0), dln_b=dn.sum(0), dwc1=dh.T @ n,
                   dbc1=dh.sum(0), dwc2=dt.T @ a, dbc2=dt.sum(0), dws0=de.T @ m, dbs0=de.sum(0), dws2=dq.T @ e, dbs2=dq.sum(0),
                   dy=dy.reshape(y.shape))
        ua = (dh.abs() @ wc1.abs()) * ln_g.abs()
        S.update(dln_g=float((dn * xhat).abs().sum(0).max()), dln_b=float(dn.abs().sum(0).max()),
                 dwc1=float((dh.abs().T @ n.abs()).max()), dbc1=float(dh.abs().sum(0).max()),
                 dwc2=float((dt.abs().T @ a.abs()).max()), dbc2=float(dt.abs().sum(0).max()),
                 dws0=float((de.abs().T @ m.abs()).max()), dbs0=float(de.abs().sum(0).max()),
                 dws2=float((dq.abs().T @ e.abs()).max()), dbs2=float(dq.abs().sum(0).max()),
                 dy=float((G.abs() + rstd * (ua + ua.mean(1, keepdim=True)
                                             + xhat.abs() * (ua * xhat.abs()).mean(1, keepdim=True))).max()))
    out["S"] = S
    return out


def _compose(y, r, leaves):
    """The block from torch's own ops in the dtype of its arguments -> x2.  ``r`` - y, the long shortcut, is a constant; the
    block's own shortcut y carries a gradient."""
    x0 = (r - y).detach()
    n = F.layer_norm(y, (y.shape[-1],), leaves["ln_g"], leaves["ln_b"], LN_EPS)
    t = F.linear(F.leaky_relu(F.linear(n, leaves["wc1"], leaves["bc1"]), SLOPE), leaves["wc2"], leaves["bc2"])
    s = torch.sigmoid(F.linear(F.relu(F.linear(t.mean(dim=(1, 2)), leaves["ws0"], leaves["bs0"])), leaves["ws2"], leaves["bs2"]))
    return t * s[:, None, None, :] + y + x0


def autograd64(y, r, p, g):
    """The same gradients from float64 autograd over torch's own ops -> dict GRADS."""
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    yy = y.double().clone().requires_grad_()
    (_compose(yy, r.double(), leaves) * g.double()).sum().backward()
    out = {"d" + k: leaves[k].grad for k in PARAMS}
    out["dy"] = yy.grad
    return out


def compose_f32(y, r, p, g=None, want_dy=True):
    """The float32 torch-op composition on the tensors' device (what tools/bench_tail_train.py times) -> (x2, dict GRADS or
    None)."""
    leaves = {k: p[k].detach().clone().requires_grad_(g is not None) for k in PARAMS}
    yy = y.detach().clone().requires_grad_(g is not None and want_dy)
    x2 = _compose(yy, r, leaves)
    if g is None:
        return x2, None
    x2.backward(g)
    grads = {"d" + k: leaves[k].grad for k in PARAMS}
    grads["dy"] = yy.grad
    return x2.detach(), grads


def kink_distances(res):
    """(LeakyReLU, SE ReLU): the smallest |pre-activation| that is not exactly zero."""
    return H.kink_distance(res["h"]), H.kink_distance(res["se_pre"])


def params_of(sd, stage=4):
    """The ten parameters of ``down<stage>``'s block out of a detector state dict -> dict PARAMS."""
    return {k: sd[f"down{stage}.{_SD_BLOCK}{n}"].detach().clone().float() for k, n in SD_NAMES.items()}


# ---- the shape sweep --------------------------------------------------------------------------------------------------------
def sweep_params(seed, c=256):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)            # noqa: E731
    h = c // 4
    return {"ln_g": 1 + 0.3 * rn(c), "ln_b": 0.2 * rn(c), "wc1": rn(c, c) / c ** 0.5, "bc1": 0.2 * rn(c), "wc2": rn(c, c) / c ** 0.5,
            "bc2": 0.2 * rn(c), "ws0": rn(h, c) / (c / 4) ** 0.5, "bs0": 0.3 * rn(h), "ws2": rn(c, h) / (h / 4) ** 0.5,
            "bs2": 0.5 * rn(c)}, g


def _h64(rows, p):
    n = F.layer_norm(rows.double(), (rows.shape[-1],), p["ln_g"].double(), p["ln_b"].double(), LN_EPS)
    return n @ p["wc1"].double().T + p["bc1"].double()


def redraw_rows_near_kink(y, p, draw, margin=SWEEP_MARGIN, rounds=64):
    """``y`` [N,C] with every row whose h (float64) has an element within ``margin`` of 0 drawn again by ``draw(count)``,
    until none is left.  LayerNorm makes h a function of the row alone.  -> (y, rows redrawn in each round)."""
    counts = []
    for _ in range(rounds):
        bad = (_h64(y, p).abs() < margin).any(1)
        k = int(bad.sum())
        if k == 0:
            return y, counts
        counts.append(k)
        y[bad] = draw(k)
    raise AssertionError("rows near the LeakyReLU kink remain")


def sweep_case(shape, seed, device=None, c=256):
    """Seeded general float32 inputs for a shape at width ``c`` -> (y, r, params, g = dx2), on the CPU.  No h within SWEEP_MARGIN of 0 (rows
    redrawn), no SE pre-activation within SWEEP_MARGIN of 0 (bs0 redrawn; asserted): a float32 rounding of a pre-activation
    across 0 would change a slope by 0.8 (LeakyReLU) or 1 (ReLU) of a whole term at any tolerance, and float32 moves h by
    3.3e-6 at most here.

    ``device``: every value is drawn on the CPU generator, in the same order, and moved there at once, so that the float64
    checks of the two margins -- restate64 several times over -- and everything after them run where the tensors are (a shape
    of tens of thousands of pixels)."""
    b, hc, wc = shape
    n_pix = b * hc * wc
    p, g = sweep_params(seed, c)
    p = T.to_device(p, device)
    on = lambda t: T.to_device(t, device)                  # noqa: E731

    def draw(k):
        return on(torch.randn((k, c), generator=g) * (0.5 + torch.rand((k, 1), generator=g)) + 0.3 * torch.randn((k, 1), generator=g))

    y, _ = redraw_rows_near_kink(draw(n_pix), p, draw)
    y = y.reshape(b, hc, wc, c)
    r = y + on(torch.randn(y.shape, generator=g)).clamp(min=0)
    dx2 = on(torch.randn(y.shape, generator=g) / n_pix)
    for _ in range(64):
        if float(restate64(y, r, p)["se_pre"].abs().min()) >= SWEEP_MARGIN:
            break
        p["bs0"] = on(0.3 * torch.randn((c // 4,), generator=g))
    assert float(restate64(y, r, p)["se_pre"].abs().min()) >= SWEEP_MARGIN
    return y, r, p, dx2


# ---- the fixture cases --------------------------------------------------------------------------------------------------------
def model_inputs():
    """Case ``model`` without its stored y, r: the block of synth.synthetic_state_dict(0), the seeded image the recorder feeds to
    the reference's network (head_train_common.model_inputs) and the seeded dlogits -> (image, params, dlogits, head params)."""
    from balf_amd.utils import synth
    image, hp, dlogits, running = H.model_inputs()
    return image, params_of(synth.synthetic_state_dict(0)), dlogits, (hp, running)


EDGES_SHAPE = (3, 3, 5)
EDGES_LN_G0 = 5                             # the channel with ln_g = 0
EDGES_CONST_ROW = (1, 2, 3)                 # the pixel whose channels are all 0.5: var = 0, xhat = 0, rstd = 1 / sqrt(eps)
EDGES_H0 = 8                                # ln_b = 0 and bc1 = 0 on channels 0..7: h == 0 exactly there on the constant row
EDGES_E0 = 7                                # the SE hidden unit with ws0 row and bs0 zero: e == 0 exactly
EDGES_SAT = ((11, 30.0), (12, -30.0))       # (channel, bs2): the saturated sigmoids
RECORD_WHOLE = 1 << 14                      # a reference result with more elements than this is recorded on some rows only


def edges_inputs(c=256):
    """Case ``edges`` at width ``c`` -> (y, r, params, g = dx2): the sweep's generator on EDGES_SHAPE with the edges named above
    (the same places at every width; all lie below 32)."""
    p, g = sweep_params(4242, c)
    p["ln_g"][EDGES_LN_G0] = 0.0
    p["ln_b"][:] = 0.0
    p["bc1"][:EDGES_H0] = 0.0
    p["ws0"][EDGES_E0] = 0.0
    p["bs0"][EDGES_E0] = 0.0
    for ch, v in EDGES_SAT:
        p["bs2"][ch] = v
    b, hc, wc = EDGES_SHAPE
    n_pix = b * hc * wc

    def draw(k):
        return 4 * torch.randn((k, c), generator=g) + torch.randn((k, 1), generator=g)

    y, _ = redraw_rows_near_kink(draw(n_pix), p, draw)
    y = y.reshape(b, hc, wc, c)
    y[EDGES_CONST_ROW] = 0.5
    r = y + torch.randn(y.shape, generator=g).clamp(min=0)
    dx2 = torch.randn(y.shape, generator=g) / n_pix
    return y, r, p, dx2


def regenerated_inputs_digest(name):
    return inputs_digest(*(model_inputs() if name == "model" else edges_inputs()))


def fixture_case(fx, name):
    """-> (y, r, params, g = dx2) of a fixture case, float32 on the CPU.  Case ``model`` stores y, r and the dx2 that the
    reference's own head sent back."""
    if name == "model":
        return (torch.from_numpy(fx["model.y"]), torch.from_numpy(fx["model.r"]), model_inputs()[1], torch.from_numpy(fx["model.dx2"]))
    return edges_inputs()


recorded_part = functools.partial(T.recorded_part, whole=RECORD_WHOLE, every=4)
recorded = functools.partial(T.recorded, part=recorded_part)


# ---- the float64 restatement of train_head with a TrainableTail ---------------------------------------------------------------
def train64(chunk, p, hp, running, presentations, lr=1e-3):
    """As head_train_common.train64 with the block in front: ``chunk`` a list of ((y, r) src, (y, r) dst, heat_src, heat_dst) CPU
    tensors, Adam over float64 copies of the ten parameters ``p`` and the head's six ``hp`` -> the per-presentation mean
    losses."""
    from tests import detector_loss_common as D
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    hl = {k: hp[k].double().clone().requires_grad_() for k in H.PARAMS}
    rm, rv = running[0].double().clone(), running[1].double().clone()
    opt = torch.optim.Adam(list(leaves.values()) + list(hl.values()), lr=lr)      # (the order of TrainableTail.parameters())
    means = []
    for _ in range(presentations):
        losses = []
        for src, dst, heat_src, heat_dst in chunk:
            opt.zero_grad()
            total = 0.0
            for (y, r), heat in ((src, heat_src), (dst, heat_dst)):
                x2 = _compose(y.double(), r.double(), leaves)
                z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
                logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
                res = D.restate64(logits.detach(), heat.float(), None, None)
                logits.backward(torch.from_numpy(res["grad"]))
                total += float(res["loss"])
            opt.step()
            losses.append(total)
        means.append(float(np.mean(losses)))
    return means
