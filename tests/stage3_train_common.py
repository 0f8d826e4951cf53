"""Shared by tests/test_stage3_train_host.py, tests/test_stage3_train_gpu.py, tests/test_stage3_guard_gpu.py,
tests/golden/make_stage3_train_golden.py and tools/bench_stage3_train.py: the fixture stage3_train.npz; the float64 restatements,
at a channel width C taken from the input, of the channel-attention block and of the multi-axis gated-MLP layer (the equations
of include/balf_hip.h, as rcab_train_common / gmlp_train_common state them at 256), of the 2 x 2 max-pool, and of the whole of
stages 3-4 and the head chained from them; the same through float64 autograd over torch's own ops; the float32 torch-op
composition; the seeded case generators at C = 128; and a Python restatement of the units' buffer layouts."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import gmlp_train_common as Gc
from tests import head_train_common as H
from tests import linrelu_train_common as Lc
from tests import rcab_train_common as Rc
from tests import train_common as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage3_train.npz")
C3 = 128                                    # stage 3's width
TOL_FLOOR = H.TOL_FLOOR
LN_EPS, SLOPE = 1e-5, 0.2
KINK_FACTOR = 8.0                           # see assert_kink_margin
POOL_FACTOR = 8.0                           # two values of a 2 x 2 window lie at least this many float32 movements of pre apart
RCAB_PARAMS, RCAB_GRADS, RCAB_GATED = Rc.PARAMS, Rc.GRADS, Rc.GATED
GMLP_PARAMS, GMLP_GRADS, GMLP_GATED = Gc.PARAMS, Gc.GRADS, Gc.GATED
RCAB_CASES, GMLP_CASES = ("model", "edges"), ("model", "layout", "edges")
RCAB_SD = dict(zip(RCAB_PARAMS, ("norm.weight", "norm.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                                 "calayer.excite.0.weight", "calayer.excite.0.bias", "calayer.excite.2.weight",
                                 "calayer.excite.2.bias")))
_RCAB, _GMLP, _CONV0 = "residual_channel_attention_block.", "residual_split_head_multi_axis_gmlp_layer.", "conv.0."
# the 38 tensors of TrainableStage3 inside down3, in the order of its parameters()
STAGE3_NAMES = ((_CONV0 + "weight", _CONV0 + "bias") + tuple(_GMLP + k for k in GMLP_PARAMS)
                + tuple(_RCAB + RCAB_SD[k] for k in RCAB_PARAMS))
STAGE_GATED = tuple("d:" + n for n in STAGE3_NAMES) + ("dx2s",)
err = Gc.err                                # train_common.err, and the exact zero where S = 0


def fixture():
    return np.load(FIXTURE)


def assert_kink_margin(h32, h64, what):
    """The margin that the recorder asserts of every ReLU / LeakyReLU pre-activation of a fixture case, exact zeros aside: with
    ``h32`` the reference's own float32 values and ``h64`` the restatement's, no element lies closer to 0 than the LARGEST
    movement |h32 - h64| of any element (that movement grows with |h|, so the elements near 0 move far less), none closer than
    KINK_FACTOR times its OWN movement, and the two masks agree.  A float32 implementation whose error is of the order of
    torch's then takes the restatement's side of every kink; an element on the other side would be an error of a whole term, at
    any tolerance."""
    move = (h32 - h64).abs()
    live = h64 != 0
    assert float(h64[live].abs().min()) > float(move.max()), (what, float(h64[live].abs().min()), float(move.max()))
    assert bool((h64[live].abs() > KINK_FACTOR * move[live]).all()), what
    assert bool(((h32 > 0) == (h64 > 0)).all()), what


def tol(fx, unit, k):
    """tol_T = max(4 d_T, the floor) of output ``k`` of ``unit`` ("rcab", "gmlp", "stage"), d_T as the recorder measured it."""
    return max(4.0 * float(fx[f"{unit}.d_{k}"]), TOL_FLOOR)


# ---- the channel-attention block at width C ------------------------------------------------------------------------------------
def rcab_restate64(y, r, p, g=None):
    """rcab_train_common.restate64 with C = y.shape[-1] channels and C / 4 squeeze-excite units in place of 256 and 64."""
    b, hc, wc, c = y.shape
    hw, n_pix = hc * wc, b * hc * wc
    Y, R = y.reshape(n_pix, c).double(), r.reshape(n_pix, c).double()
    ln_g, ln_b, wc1, bc1, wc2, bc2, ws0, bs0, ws2, bs2 = (p[k].double() for k in RCAB_PARAMS)
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
    sp = s.repeat_interleave(hw, dim=0)
    out = {"h": h, "se_pre": pre, "x2": (t * sp + R).reshape(y.shape)}
    S = {"x2": float((((a.abs() @ wc2.abs().T) + bc2.abs()) * sp + R.abs()).max())}
    if g is not None:
        G = g.reshape(n_pix, c).double()
        ds = (G * t).reshape(b, hw, c).sum(1)
        dq = ds * s * (1 - s)
        de = (dq @ ws2) * (pre > 0)
        dm = de @ ws0
        dt = G * sp + (dm / hw).repeat_interleave(hw, dim=0)
        dh = (dt @ wc2) * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, SLOPE))
        dn = dh @ wc1
        u = dn * ln_g
        dy = G + rstd * (u - u.mean(1, keepdim=True) - xhat * (u * xhat).mean(1, keepdim=True))
        out.update(dln_g=(dn * xhat).sum(0), dln_b=dn.sum(0), dwc1=dh.T @ n, dbc1=dh.sum(0), dwc2=dt.T @ a, dbc2=dt.sum(0),
                   dws0=de.T @ m, dbs0=de.sum(0), dws2=dq.T @ e, dbs2=dq.sum(0), dy=dy.reshape(y.shape))
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


def rcab_compose(y, r, leaves):
    """The block from torch's own ops in the dtype of its arguments -> x2; ``r`` - y, the long shortcut, is a constant."""
    c = y.shape[-1]
    n = F.layer_norm(y, (c,), leaves["ln_g"], leaves["ln_b"], LN_EPS)
    t = F.linear(F.leaky_relu(F.linear(n, leaves["wc1"], leaves["bc1"]), SLOPE), leaves["wc2"], leaves["bc2"])
    s = torch.sigmoid(F.linear(F.relu(F.linear(t.mean(dim=(1, 2)), leaves["ws0"], leaves["bs0"])), leaves["ws2"], leaves["bs2"]))
    return t * s[:, None, None, :] + y + (r - y).detach()


def rcab_autograd64(y, r, p, g):
    leaves = {k: p[k].double().clone().requires_grad_() for k in RCAB_PARAMS}
    yy = y.double().clone().requires_grad_()
    (rcab_compose(yy, r.double(), leaves) * g.double()).sum().backward()
    return dict({"d" + k: leaves[k].grad for k in RCAB_PARAMS}, dy=yy.grad)


def rcab_params_of(sd, stage=3):
    return {k: sd[f"down{stage}.{_RCAB}{n}"].detach().clone().float() for k, n in RCAB_SD.items()}


def rcab_sweep_params(seed, c=C3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)            # noqa: E731
    h = c // 4
    return {"ln_g": 1 + 0.3 * rn(c), "ln_b": 0.2 * rn(c), "wc1": rn(c, c) / c ** 0.5, "bc1": 0.2 * rn(c), "wc2": rn(c, c) / c ** 0.5,
            "bc2": 0.2 * rn(c), "ws0": rn(h, c) / (c / 4) ** 0.5, "bs0": 0.3 * rn(h), "ws2": rn(c, h) / (h / 4) ** 0.5,
            "bs2": 0.5 * rn(c)}, g


def _rcab_h64(rows, p):
    n = F.layer_norm(rows.double(), (rows.shape[-1],), p["ln_g"].double(), p["ln_b"].double(), LN_EPS)
    return n @ p["wc1"].double().T + p["bc1"].double()


def _redraw_rows(y, p, draw, margin=Rc.SWEEP_MARGIN):
    """rcab_train_common.redraw_rows_near_kink at the width of ``y``: LayerNorm makes h a function of the row alone."""
    for _ in range(64):
        bad = (_rcab_h64(y, p).abs() < margin).any(1)
        if not int(bad.sum()):
            return y
        y[bad] = draw(int(bad.sum()))
    raise AssertionError("rows near the LeakyReLU kink remain")


def rcab_sweep_case(shape, seed, device=None, c=C3):
    """rcab_train_common.sweep_case at width ``c`` -> (y, r, params, g = dx2): no h and no squeeze-excite pre-activation within
    rcab_train_common.SWEEP_MARGIN of its kink."""
    b, hc, wc = shape
    n_pix = b * hc * wc
    p, g = rcab_sweep_params(seed, c)
    p = T.to_device(p, device)
    on = lambda t: T.to_device(t, device)                  # noqa: E731

    def draw(k):
        return on(torch.randn((k, c), generator=g) * (0.5 + torch.rand((k, 1), generator=g)) + 0.3 * torch.randn((k, 1), generator=g))

    y = _redraw_rows(draw(n_pix), p, draw).reshape(b, hc, wc, c)
    r = y + on(torch.randn(y.shape, generator=g)).clamp(min=0)
    dx2 = on(torch.randn(y.shape, generator=g) / n_pix)
    for _ in range(64):
        if float(rcab_restate64(y, r, p)["se_pre"].abs().min()) >= Rc.SWEEP_MARGIN:
            break
        p["bs0"] = on(0.3 * torch.randn((c // 4,), generator=g))
    assert float(rcab_restate64(y, r, p)["se_pre"].abs().min()) >= Rc.SWEEP_MARGIN
    return y, r, p, dx2


def rcab_edges_inputs(c=C3):
    """rcab_train_common.edges_inputs at width ``c``: a constant row, a zero ln_g channel, exact zeros of h, a dead squeeze-excite
    unit, saturated sigmoids (the same places; all lie below 32)."""
    p, g = rcab_sweep_params(4242, c)
    p["ln_g"][Rc.EDGES_LN_G0] = 0.0
    p["ln_b"][:] = 0.0
    p["bc1"][:Rc.EDGES_H0] = 0.0
    p["ws0"][Rc.EDGES_E0] = 0.0
    p["bs0"][Rc.EDGES_E0] = 0.0
    for ch, v in Rc.EDGES_SAT:
        p["bs2"][ch] = v
    b, hc, wc = Rc.EDGES_SHAPE
    n_pix = b * hc * wc

    def draw(k):
        return 4 * torch.randn((k, c), generator=g) + torch.randn((k, 1), generator=g)

    y = _redraw_rows(draw(n_pix), p, draw).reshape(b, hc, wc, c)
    y[Rc.EDGES_CONST_ROW] = 0.5
    r = y + torch.randn(y.shape, generator=g).clamp(min=0)
    return y, r, p, torch.randn(y.shape, generator=g) / n_pix


# ---- the gated-MLP layer at width C --------------------------------------------------------------------------------------------
def gmlp_restate64(x0, p, g=None):
    """gmlp_train_common.restate64 with C = x0.shape[-1] channels (2C where it has 512); the token matrices stay [64,64]."""
    b, hc, wc, c = x0.shape
    n_pix = b * hc * wc
    X = x0.reshape(n_pix, c).double()
    P = {k: p[k].double() for k in GMLP_PARAMS}
    ln, ln_bwd, phi, gelu_grad = Gc._ln64, Gc._ln64_bwd, Gc._phi, Gc._gelu_grad
    n0, xhat0, rstd0 = ln(X, P["norm.weight"], P["norm.bias"])
    h0 = n0 @ P["dense1.weight"].T + P["dense1.bias"]
    g0 = h0 * phi(h0)
    keep, outs = [], []
    for k, (layer, unit) in enumerate(Gc.BRANCHES):
        q = lambda s: P[f"{layer}.{s}"]                         # noqa: E731
        z = g0[:, c * k:c * k + c]
        nb, xhat_b, rstd_b = ln(z, q("norm.weight"), q("norm.bias"))
        hb = nb @ q("dense1.weight").T + q("dense1.bias")
        gb = hb * phi(hb)
        a, cc = gb[:, :c], gb[:, c:]
        cn, xhat_g, rstd_g = ln(cc, q(f"{unit}.norm.weight"), q(f"{unit}.norm.bias"))
        idx = Gc.token_index(b, hc, wc, grid=(k == 0)).to(X.device)
        wt, bt = q(f"{unit}.dense.weight"), q(f"{unit}.dense.bias")
        mix = torch.empty_like(cn)
        mix[idx.reshape(-1)] = (torch.einsum("pq,gqc->gpc", wt, cn[idx]) + bt[None, :, None]).reshape(-1, c)
        gated = a * (mix + 1.0)
        outs.append(z + gated @ q("dense2.weight").T + q("dense2.bias"))
        keep.append(dict(nb=nb, xhat_b=xhat_b, rstd_b=rstd_b, hb=hb, a=a, cn=cn, xhat_g=xhat_g, rstd_g=rstd_g, idx=idx, mix=mix,
                         gated=gated))
    cat = torch.cat(outs, 1)
    y = cat @ P["dense2.weight"].T + P["dense2.bias"] + X
    out = {"y": y.reshape(x0.shape), "h0": h0, "hb": [kk["hb"] for kk in keep]}
    S = {"y": float((cat.abs() @ P["dense2.weight"].abs().T + P["dense2.bias"].abs() + X.abs()).max())}
    if g is not None:
        G = g.reshape(n_pix, c).double()

        def put(name, value, scale):
            out["d:" + name], S["d:" + name] = value, float(scale.max())

        put("dense2.bias", G.sum(0), G.abs().sum(0))
        put("dense2.weight", G.T @ cat, G.abs().T @ cat.abs())
        dcat = G @ P["dense2.weight"]
        dg0 = []
        for k, (layer, unit) in enumerate(Gc.BRANCHES):
            q = lambda s: P[f"{layer}.{s}"]                     # noqa: E731
            kk = keep[k]
            dz1 = dcat[:, c * k:c * k + c]
            put(f"{layer}.dense2.bias", dz1.sum(0), dz1.abs().sum(0))
            put(f"{layer}.dense2.weight", dz1.T @ kk["gated"], dz1.abs().T @ kk["gated"].abs())
            dgated = dz1 @ q("dense2.weight")
            da, dmix = dgated * (kk["mix"] + 1.0), dgated * kk["a"]
            idx = kk["idx"]
            dm_g, cn_g = dmix[idx], kk["cn"][idx]               # [G,64,C]
            put(f"{layer}.{unit}.dense.bias", dm_g.sum((0, 2)), dm_g.abs().sum((0, 2)))
            put(f"{layer}.{unit}.dense.weight", torch.einsum("gpc,gqc->pq", dm_g, cn_g),
                torch.einsum("gpc,gqc->pq", dm_g.abs(), cn_g.abs()))
            dcn = torch.empty_like(dmix)
            dcn[idx.reshape(-1)] = torch.einsum("pq,gpc->gqc", q(f"{unit}.dense.weight"), dm_g).reshape(-1, c)
            dc, dgain, dbias, _ = ln_bwd(dcn, kk["xhat_g"], kk["rstd_g"], q(f"{unit}.norm.weight"))
            put(f"{layer}.{unit}.norm.weight", dgain, (dcn * kk["xhat_g"]).abs().sum(0))
            put(f"{layer}.{unit}.norm.bias", dbias, dcn.abs().sum(0))
            dhb = torch.cat([da, dc], 1) * gelu_grad(kk["hb"])
            put(f"{layer}.dense1.bias", dhb.sum(0), dhb.abs().sum(0))
            put(f"{layer}.dense1.weight", dhb.T @ kk["nb"], dhb.abs().T @ kk["nb"].abs())
            dnb = dhb @ q("dense1.weight")
            dz, dgain, dbias, _ = ln_bwd(dnb, kk["xhat_b"], kk["rstd_b"], q("norm.weight"))
            put(f"{layer}.norm.weight", dgain, (dnb * kk["xhat_b"]).abs().sum(0))
            put(f"{layer}.norm.bias", dbias, dnb.abs().sum(0))
            dg0.append(dz1 + dz)
        dh0 = torch.cat(dg0, 1) * gelu_grad(h0)
        put("dense1.bias", dh0.sum(0), dh0.abs().sum(0))
        put("dense1.weight", dh0.T @ n0, dh0.abs().T @ n0.abs())
        dn0 = dh0 @ P["dense1.weight"]
        dx, dgain, dbias, _ = ln_bwd(dn0, xhat0, rstd0, P["norm.weight"])
        put("norm.weight", dgain, (dn0 * xhat0).abs().sum(0))
        put("norm.bias", dbias, dn0.abs().sum(0))
        _, _, _, mag = ln_bwd(dh0.abs() @ P["dense1.weight"].abs(), xhat0.abs(), rstd0, P["norm.weight"].abs())
        out["dx0"], S["dx0"] = (G + dx).reshape(x0.shape), float((G.abs() + mag).max())
    out["S"] = S
    return out


def gmlp_compose(x0, leaves):
    """The layer from oracle.oracle's own arithmetic in the dtype of its arguments -> y, at the width of ``x0``."""
    c = x0.shape[-1]
    sd = {"L." + k: v for k, v in leaves.items()}
    t = F.gelu(oracle._lin(sd, "L.dense1", oracle._ln(sd, "L.norm", x0)))
    u = oracle._gmlp_branch(sd, "L.grid_gmlp_layer", "grid_gating_unit", t[..., :c], True)
    v = oracle._gmlp_branch(sd, "L.block_gmlp_layer", "block_gating_unit", t[..., c:], False)
    return oracle._lin(sd, "L.dense2", torch.cat([u, v], dim=-1)) + x0


def gmlp_autograd64(x0, p, g):
    leaves = {k: p[k].double().clone().requires_grad_() for k in GMLP_PARAMS}
    xx = x0.double().clone().requires_grad_()
    (gmlp_compose(xx, leaves) * g.double()).sum().backward()
    return dict({"d:" + k: leaves[k].grad for k in GMLP_PARAMS}, dx0=xx.grad)


def gmlp_params_of(sd, stage=3):
    return {k: sd[f"down{stage}.{_GMLP}{k}"].detach().clone().float() for k in GMLP_PARAMS}


def gmlp_sweep_case(shape, seed, device=None, c=C3):
    """gmlp_train_common.sweep_case at width ``c`` -> (x0, params, g = dy)."""
    from balf_amd import ops
    b, hc, wc = shape
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, shp in ops.gmlp_param_shapes(c).items():
        if k.rsplit(".", 2)[-2] == "norm":
            p[k] = 1 + 0.3 * torch.randn(shp, generator=g) if k.endswith("weight") else 0.2 * torch.randn(shp, generator=g)
        elif len(shp) == 2:
            p[k] = torch.randn(shp, generator=g) / shp[1] ** 0.5
        else:
            p[k] = 0.2 * torch.randn(shp, generator=g)
    x0 = (torch.randn((b, hc, wc, c), generator=g) * (0.5 + torch.rand((b, hc, wc, 1), generator=g)) + 0.3).clamp(min=0)
    dy = torch.randn(x0.shape, generator=g) / (b * hc * wc)
    return T.to_device((x0, p, dy), device)


GMLP_EDGES_SAT = ((3, 9.0), (4, -9.0), (150, 9.0), (151, -9.0))    # (channel of a dense1 output, bias): one pair in each half


def gmlp_layout_inputs(c=C3):
    return gmlp_sweep_case(Gc.LAYOUT_SHAPE, 2718, c=c)


def gmlp_edges_inputs(c=C3):
    """gmlp_train_common.edges_inputs at width ``c``: a constant row, a constant c half in the grid branch, a closed gate, zero
    gains, saturated GELUs."""
    x0, p, dy = gmlp_sweep_case(Gc.EDGES_SHAPE, 4242, c=c)
    x0[Gc.EDGES_CONST_ROW] = 0.5
    (gl, gu), (bl, bu) = Gc.BRANCHES
    p[f"{gl}.dense1.weight"][c:] = 0.0
    p[f"{gl}.dense1.bias"][c:] = Gc.EDGES_C_BIAS
    p[f"{bl}.{bu}.dense.weight"][Gc.EDGES_GATE0] = 0.0
    p[f"{bl}.{bu}.dense.bias"][Gc.EDGES_GATE0] = -1.0
    for k in (f"{gl}.norm.weight", f"{gl}.{gu}.norm.weight", "norm.weight"):
        p[k][Gc.EDGES_GAIN0] = 0.0
    for k in ("dense1.bias", f"{bl}.dense1.bias"):
        for ch, v in GMLP_EDGES_SAT:
            p[k][ch] = v
    return x0, p, dy


# ---- the 2 x 2 max-pool ---------------------------------------------------------------------------------------------------------
def pool_reference(x, g=None):
    """torch's CPU max_pool2d on NHWC ``x`` [B,H,W,C] -> (out [B,H/2,W/2,C], which uint8 0..3, dx or None): the reference of the
    pool unit, bit for bit, in the dtype of ``x``."""
    xx = x.detach().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(g is not None)
    out, idx = F.max_pool2d(xx, 2, return_indices=True)
    w = x.shape[2]
    which = ((idx // w) % 2 * 2 + (idx % w) % 2).to(torch.uint8)
    dx = None
    if g is not None:
        out.backward(g.detach().cpu().permute(0, 3, 1, 2).contiguous())
        dx = xx.grad.permute(0, 2, 3, 1).contiguous()
    return out.detach().permute(0, 2, 3, 1).contiguous(), which.permute(0, 2, 3, 1).contiguous(), dx


def pool_gap(x):
    """The smallest distance between the largest and the second largest value of a 2 x 2 window of NHWC ``x``."""
    b, h, w, c = x.shape
    win = x.reshape(b, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    top = win.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def pool_cases(shape, c, seed):
    """name -> x [B,2Ho,2Wo,C] for an OUTPUT map ``shape`` = (B, Ho, Wo): random values, a constant (every window a four-way tie),
    signed zeros, infinities, and a NaN at each window position in turn (with a second NaN in front of it in some windows)."""
    b, ho, wo = shape
    g = torch.Generator().manual_seed(seed)
    full = (b, 2 * ho, 2 * wo, c)
    cases = {"random": torch.randn(full, generator=g), "constant": torch.full(full, 0.75)}
    sign = torch.randint(0, 2, full, generator=g).float() * 2 - 1
    cases["zeros"] = torch.zeros(full) * sign                                       # +0 and -0
    inf = torch.randn(full, generator=g)
    kind = torch.randint(0, 6, full, generator=g)
    inf[kind == 0], inf[kind == 1] = float("inf"), float("-inf")
    cases["inf"] = inf
    for pos in range(4):
        x = torch.randn(full, generator=g)
        view = x.reshape(b, ho, 2, wo, 2, c)
        view[:, :, pos // 2, :, pos % 2, :] = float("nan")
        if pos:
            first = torch.rand((b, ho, wo, c), generator=g) < 0.5
            view[:, :, 0, :, 0, :][first] = float("nan")
        cases[f"nan{pos}"] = x
    return cases


# ---- all of stages 3-4 and the head --------------------------------------------------------------------------------------------
def stage_params(sd):
    """What stage64 and the recorder take out of a detector state dict."""
    hp, running = H.params_of(sd)
    return {3: ((sd["down3.conv.0.weight"].float(), sd["down3.conv.0.bias"].float()), gmlp_params_of(sd, 3), rcab_params_of(sd, 3)),
            4: ((sd["down4.conv.0.weight"].float(), sd["down4.conv.0.bias"].float()), gmlp_params_of(sd, 4), rcab_params_of(sd, 4)),
            "head": hp, "running": running}


def stage64(x2s, sp, dlogits):
    """The float64 restatement of TrainableStage3 in training mode, chained from the units' closed formulas: ``x2s``
    [B,H4,W4,64], ``sp`` = stage_params(sd), ``dlogits`` [B,65,H4/4,W4/4] -> the outputs under STAGE_GATED, ``S`` with each one's
    scale (that of the unit that makes it), ``logits``, the inputs of the units of stage 3 (``x0``, ``y``, ``r``, ``pre``, ``dpre``,
    ``dy``), and ``kinks``: name -> the pre-activation of every ReLU / LeakyReLU on the way."""
    def down(x, stage):
        (w, b), gp, rp = sp[stage]
        lin = Lc.restate64(x, w, b)
        x0 = lin["y"].reshape(x.shape[:3] + (w.shape[0],))
        gm = gmlp_restate64(x0, gp)
        rc = rcab_restate64(gm["y"], gm["y"] + x0, rp)
        return x0, gm["y"], rc["x2"], {f"down{stage}.conv.0": lin["h"], f"down{stage}.rcab.conv1": rc["h"],
                                       f"down{stage}.rcab.excite.0": rc["se_pre"]}

    x0, y, pre, kinks = down(x2s.double(), 3)
    x3, which, _ = pool_reference(pre)
    x0_4, y_4, x2, k4 = down(x3, 4)
    kinks.update(k4)
    head = H.restate64(x2, sp["head"], dlogits)
    kinks["down4.conv2"] = head["h"]
    out = {"logits": head["logits"], "x0": x0, "y": y, "r": y + x0, "pre": pre, "kinks": kinks, "pool_gap": pool_gap(pre)}
    S = {}

    def up(x, x0, y, g, stage):
        """the backward of a Down stage from the gradient ``g`` at its (pre-pool) output -> dx, and its 38 gradients"""
        (w, b), gp, rp = sp[stage]
        rc = rcab_restate64(y, y + x0, rp, g)
        gm = gmlp_restate64(x0, gp, rc["dy"])
        lin = Lc.restate64(x, w, b, gm["dx0"].reshape(g.shape) + g)        # the layer and its shortcut, and the long shortcut
        if stage == 3:
            for name, val, scale in ((_CONV0 + "weight", lin["dw"], lin["S"]["dw"]), (_CONV0 + "bias", lin["db"], lin["S"]["db"])):
                out["d:" + name], S["d:" + name] = val, scale
            for k in GMLP_PARAMS:
                out["d:" + _GMLP + k], S["d:" + _GMLP + k] = gm["d:" + k], gm["S"]["d:" + k]
            for k in RCAB_PARAMS:
                out["d:" + _RCAB + RCAB_SD[k]], S["d:" + _RCAB + RCAB_SD[k]] = rc["d" + k], rc["S"]["d" + k]
            out["dy"] = rc["dy"]
        return lin["dx"].reshape(x.shape), lin["S"]["dx"]

    dx3, _ = up(x3, x0_4, y_4, head["dx2"], 4)
    sel = F.one_hot(which.long(), 4).permute(0, 1, 2, 4, 3).double()       # [B,Ho,Wo,4,C]
    b, ho, wo, c = dx3.shape
    dpre = (sel * dx3[:, :, :, None, :]).reshape(b, ho, wo, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * ho, 2 * wo, c)
    out["dpre"] = dpre
    out["dx2s"], S["dx2s"] = up(x2s.double(), x0, y, dpre, 3)
    out["S"] = S
    return out


def stage_compose(x2s, leaves):
    """Stages 3-4 from torch's own ops in the dtype of the arguments -> x2 of down4; ``leaves``: {3, 4} -> ((w, b), gMLP leaves,
    RCAB leaves)."""
    x = x2s
    for stage in (3, 4):
        (w, b), gl, rl = leaves[stage]
        x0 = F.relu(F.linear(x, w, b))
        y = gmlp_compose(x0, gl)
        x = rcab_compose(y, (y + x0).detach(), rl) + (x0 - x0.detach())
        if stage == 3:
            x = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    return x


def _leaves(sp, requires_grad=True):
    def leaf(t):
        return t.double().clone().requires_grad_(requires_grad)
    return {s: (tuple(leaf(t) for t in sp[s][0]), {k: leaf(v) for k, v in sp[s][1].items()}, {k: leaf(v) for k, v in sp[s][2].items()})
            for s in (3, 4)}


def _leaf_list(leaves, hl):
    """the order of TrainableStage3.parameters(): down3, then stage 4 (conv.0, the layer, the block), then the head"""
    out = []
    for s in (3, 4):
        (w, b), gl, rl = leaves[s]
        out += [w, b] + [gl[k] for k in GMLP_PARAMS] + [rl[k] for k in RCAB_PARAMS]
    return out + [hl[k] for k in H.PARAMS]


def stage_autograd64(x2s, sp, dlogits):
    """The gradients of stage64 from float64 autograd over torch's own ops -> dict STAGE_GATED."""
    leaves = _leaves(sp)
    hl = {k: sp["head"][k].double().clone().requires_grad_() for k in H.PARAMS}
    xx = x2s.double().clone().requires_grad_()
    x2 = stage_compose(xx, leaves)
    z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
    logits = F.batch_norm(z, None, None, hl["gamma"], hl["beta"], training=True, momentum=0.0, eps=H.EPS)
    (logits * dlogits.double()).sum().backward()
    (w, b), gl, rl = leaves[3]
    out = {"d:" + _CONV0 + "weight": w.grad, "d:" + _CONV0 + "bias": b.grad, "dx2s": xx.grad}
    out.update({"d:" + _GMLP + k: gl[k].grad for k in GMLP_PARAMS})
    out.update({"d:" + _RCAB + RCAB_SD[k]: rl[k].grad for k in RCAB_PARAMS})
    return out


def train64(chunk, sp, presentations, lr=1e-3):
    """linrelu_train_common.train64 with stage 3 in front: ``chunk`` a list of (x2s src, x2s dst, heat_src, heat_dst) CPU tensors,
    Adam over float64 copies of the 82 tensors in the order of TrainableStage3.parameters() -> the per-presentation mean losses."""
    from tests import detector_loss_common as D
    leaves = _leaves(sp)
    hl = {k: sp["head"][k].double().clone().requires_grad_() for k in H.PARAMS}
    rm, rv = sp["running"][0].double().clone(), sp["running"][1].double().clone()
    opt = torch.optim.Adam(_leaf_list(leaves, hl), lr=lr)
    means = []
    for _ in range(presentations):
        losses = []
        for src, dst, heat_src, heat_dst in chunk:
            opt.zero_grad()
            total = 0.0
            for x2s, heat in ((src, heat_src), (dst, heat_dst)):
                x2 = stage_compose(x2s.double(), leaves)
                z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
                logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
                res = D.restate64(logits.detach(), heat.float(), None, None)
                logits.backward(torch.from_numpy(res["grad"]))
                total += float(res["loss"])
            opt.step()
            losses.append(total)
        means.append(float(np.mean(losses)))
    return means


def stage_compose_f32(x2s, sp, dlogits):
    """The float32 torch-op composition of stages 3-4 and the head on the tensors' device, forward and backward (what
    tools/bench_stage3_train.py times) -> logits."""
    def leaf(t):
        return t.detach().clone().requires_grad_()
    leaves = {s: (tuple(leaf(t) for t in sp[s][0]), {k: leaf(v) for k, v in sp[s][1].items()}, {k: leaf(v) for k, v in sp[s][2].items()})
              for s in (3, 4)}
    hl = {k: leaf(sp["head"][k]) for k in H.PARAMS}
    x2 = stage_compose(x2s.detach().clone().requires_grad_(), leaves)
    z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
    logits = F.batch_norm(z, None, None, hl["gamma"], hl["beta"], training=True, momentum=0.0, eps=H.EPS)
    logits.backward(dlogits)
    return logits.detach()


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def stage_inputs(fx):
    """Case ``stage`` -> (x2s, stage_params of synth.synthetic_state_dict(0), dlogits): the reference's own stage-2 output on the
    seeded image and the gradient of the reference's loss, both stored."""
    from balf_amd.utils import synth
    return torch.from_numpy(fx["stage.x2s"]), stage_params(synth.synthetic_state_dict(0)), torch.from_numpy(fx["stage.dlogits"])


@functools.lru_cache(maxsize=None)
def _stage_res():
    return stage64(*stage_inputs(fixture()))


def rcab_case(name):
    """-> (y, r, params, g = dx2) of a fixture case at C = 128, float32 on the CPU.  Case ``model``: the float32 roundings of the
    restatement's own y, r and dpre of case ``stage`` (computed here, not stored), with the block of synth.synthetic_state_dict(0)."""
    if name == "model":
        res, sp = _stage_res(), stage_inputs(fixture())[1]
        return res["y"].float(), res["r"].float(), sp[3][2], res["dpre"].float()
    return rcab_edges_inputs()


def gmlp_case(name):
    """-> (x0, params, g = dy) of a fixture case at C = 128; ``model`` as in rcab_case, from x0 and dy of case ``stage``."""
    if name == "model":
        res, sp = _stage_res(), stage_inputs(fixture())[1]
        return res["x0"].float(), sp[3][1], res["dy"].reshape(res["x0"].shape).float()
    return gmlp_layout_inputs() if name == "layout" else gmlp_edges_inputs()


RECORD_WHOLE = 1 << 12
recorded_part = functools.partial(T.recorded_part, whole=RECORD_WHOLE, every=32)


# ---- the buffer layouts, restated (rcab_train.hip, gmlp_train.hip, pool_train.hip: make_layout) --------------------------------
def _al(nbytes):
    return -(-nbytes // 256) * 256


def unit_sizes(unit, c, b, h, w):
    """(workspace bytes, saved bytes) of balf_train_unit_sizes for sizes inside the limits: every region rounded up to 256."""
    n = b * h * w
    rows, s, _, pc = T.pixel_slices(n)
    act = n * c * 4
    if unit == "rcab":
        _, pi = T.rcab_image_blocks(h * w)
        saved = 3 * _al(act) + _al(n * 8) + _al(b * c * 8) + _al(b * c // 4 * 8) + _al(b * c * 8) + _al(b * c * 4)
        work = (_al(b * pi * c * 8) + _al(2 * pc * c * 8) + _al(b * c * 8) + _al(b * c // 4 * 8) + _al(b * c * 4) + 2 * _al(act)
                + _al(s * c * c * 4))
        return work, saved
    if unit == "gmlp":
        _, _, pw = T.gmlp_mix_groups(n)
        st = _al(n * 8)
        saved = _al(act) + st + 3 * _al(2 * act) + 2 * (_al(act) + st + 2 * _al(2 * act) + st + 3 * _al(act))
        work = (_al(2 * pc * 2 * c * 8) + _al(c // 64 * pw * (64 * 64 + 64) * 8) + 3 * _al(2 * act) + 2 * _al(act)
                + _al(s * 2 * c * c * 4))
        return work, saved
    assert unit == "pool"
    return 0, b * (h // 2) * (w // 2) * c
