"""Shared by tests/test_gmlp_train_host.py, tests/test_gmlp_train_gpu.py, tests/golden/make_gmlp_train_golden.py and
tools/bench_gmlp_train.py, and by the stage-3 tests through tests/stage3_train_common.py: the fixture gmlp_train.npz, the float64
restatement of the multi-axis gated-MLP layer (include/balf_hip.h: balf_gmlp_train_forward) and of its backward as closed formulas,
the same through float64 autograd over oracle.oracle's arithmetic, the float32 torch-op composition, the error measure of the
gates, and the seeded case generators.  All of it at a width C: the last dimension of the input where there is one, ``c`` (256,
stage 4's, unless stated) in the generators; the token matrices stay [64,64]."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import head_train_common as H
from tests import rcab_train_common as R
from tests import train_common as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmlp_train.npz")
FIXTURE_CASES = ("model", "layout", "edges")
_BRANCH = ("norm.weight", "norm.bias", "dense1.weight", "dense1.bias", "{u}.norm.weight", "{u}.norm.bias", "{u}.dense.weight",
           "{u}.dense.bias", "dense2.weight", "dense2.bias")
BRANCHES = (("grid_gmlp_layer", "grid_gating_unit"), ("block_gmlp_layer", "block_gating_unit"))
PARAMS = (("norm.weight", "norm.bias", "dense1.weight", "dense1.bias")
          + tuple(f"{layer}.{n.format(u=unit)}" for layer, unit in BRANCHES for n in _BRANCH)
          + ("dense2.weight", "dense2.bias"))                   # = balf_amd.ops.GMLP_PARAMS
GRADS = tuple("d:" + k for k in PARAMS) + ("dx0",)
GATED = ("y",) + GRADS                      # the 28 outputs
TOL_FLOOR = H.TOL_FLOOR
LN_EPS = 1e-5
_SD_LAYER = "residual_split_head_multi_axis_gmlp_layer."
SD_PREFIX = "down4." + _SD_LAYER
inputs_digest = T.inputs_digest


def fixture():
    return np.load(FIXTURE)


def err(got, want64, scale):
    """max |got - want| / S, the measure of every gate (train_common.err).  S = 0 -- every term of the reduction is an exact
    zero, as the gain gradient of a LayerNorm whose input is constant on every pixel -- demands the exact zero."""
    if scale > 0:
        return T.err(got, want64, scale)
    return 0.0 if T.err(got, want64, 1.0) == 0.0 else float("inf")


def token_index(b, hc, wc, grid):
    """[groups, 64] pixel indices: row = a group, column = the token (8 * row + column of the 8 x 8 grid or block).  Grid map: the
    token is which of the 8 x 8 regions of (hc / 8) x (wc / 8) pixels, the group (image, place inside the region).  Block map: the
    token is the place inside a contiguous 8 x 8 block, the group (image, block)."""
    fh, fw = hc // 8, wc // 8
    img = torch.arange(b).reshape(b, 1, 1, 1, 1) * (hc * wc)
    t_y, t_x = torch.arange(8).reshape(1, 1, 1, 8, 1), torch.arange(8).reshape(1, 1, 1, 1, 8)
    g_y, g_x = torch.arange(fh).reshape(1, fh, 1, 1, 1), torch.arange(fw).reshape(1, 1, fw, 1, 1)
    if grid:
        pix = img + (t_y * fh + g_y) * wc + (t_x * fw + g_x)
    else:
        pix = img + (g_y * 8 + t_y) * wc + (g_x * 8 + t_x)
    return pix.reshape(b * fh * fw, 64)


def _ln64(x, g, b):
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
    xhat = (x - mean) * rstd
    return xhat * g + b, xhat, rstd


def _ln64_bwd(dn, xhat, rstd, g):
    """-> (dx, dgain, dbias, the sum of absolute values of dx's terms)"""
    u = dn * g
    dx = rstd * (u - u.mean(1, keepdim=True) - xhat * (u * xhat).mean(1, keepdim=True))
    ua = u.abs()
    mag = rstd * (ua + ua.mean(1, keepdim=True) + xhat.abs() * (ua * xhat.abs()).mean(1, keepdim=True))
    return dx, (dn * xhat).sum(0), dn.sum(0), mag


def _phi(h):
    return 0.5 * torch.special.erfc(-h / np.sqrt(2.0))


def _gelu_grad(h):
    return _phi(h) + h * torch.exp(-0.5 * h * h) / np.sqrt(2.0 * np.pi)


def restate64(x0, p, g=None):
    """The equations of include/balf_hip.h in float64 on the CPU.  ``x0`` [B,Hc,Wc,C]; ``p``: dict PARAMS; ``g`` = dy or None.
    -> dict of float64 tensors: y, the 26 gradients as "d:<name>", dx0, and ``S``: name -> the scale of the error measure, the
    largest sum of absolute values of the terms of that output's last reduction (y: |cat| |W2|^T + |b2| + |x0|; a bias gradient: sum
    |d|; a weight gradient: |d|^T |input|; a LayerNorm gain: sum |dn xhat|; dWt: sum over groups and channels of |dmix[p]| |cn[q]|;
    dx0: |g| + rstd times the three terms of the LayerNorm's backward, as dy of rcab_train_common)."""
    b, hc, wc, c = x0.shape
    n_pix = b * hc * wc
    X = x0.reshape(n_pix, c).double()
    P = {k: p[k].double() for k in PARAMS}
    n0, xhat0, rstd0 = _ln64(X, P["norm.weight"], P["norm.bias"])
    h0 = n0 @ P["dense1.weight"].T + P["dense1.bias"]
    g0 = h0 * _phi(h0)
    keep, outs = [], []
    for k, (layer, unit) in enumerate(BRANCHES):
        q = lambda s: P[f"{layer}.{s}"]                         # noqa: E731
        z = g0[:, c * k:c * k + c]
        nb, xhat_b, rstd_b = _ln64(z, q("norm.weight"), q("norm.bias"))
        hb = nb @ q("dense1.weight").T + q("dense1.bias")
        gb = hb * _phi(hb)
        a, cc = gb[:, :c], gb[:, c:]
        cn, xhat_g, rstd_g = _ln64(cc, q(f"{unit}.norm.weight"), q(f"{unit}.norm.bias"))
        idx = token_index(b, hc, wc, grid=(k == 0)).to(X.device)
        wt, bt = q(f"{unit}.dense.weight"), q(f"{unit}.dense.bias")
        mix = torch.empty_like(cn)
        mix[idx.reshape(-1)] = (torch.einsum("pq,gqc->gpc", wt, cn[idx]) + bt[None, :, None]).reshape(-1, c)
        gated = a * (mix + 1.0)
        outs.append(z + gated @ q("dense2.weight").T + q("dense2.bias"))
        keep.append(dict(z=z, nb=nb, xhat_b=xhat_b, rstd_b=rstd_b, hb=hb, a=a, c=cc, cn=cn, xhat_g=xhat_g, rstd_g=rstd_g, idx=idx,
                         mix=mix, gated=gated))
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
        for k, (layer, unit) in enumerate(BRANCHES):
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
            dc, dgain, dbias, _ = _ln64_bwd(dcn, kk["xhat_g"], kk["rstd_g"], q(f"{unit}.norm.weight"))
            put(f"{layer}.{unit}.norm.weight", dgain, (dcn * kk["xhat_g"]).abs().sum(0))
            put(f"{layer}.{unit}.norm.bias", dbias, dcn.abs().sum(0))
            dhb = torch.cat([da, dc], 1) * _gelu_grad(kk["hb"])
            put(f"{layer}.dense1.bias", dhb.sum(0), dhb.abs().sum(0))
            put(f"{layer}.dense1.weight", dhb.T @ kk["nb"], dhb.abs().T @ kk["nb"].abs())
            dnb = dhb @ q("dense1.weight")
            dz, dgain, dbias, _ = _ln64_bwd(dnb, kk["xhat_b"], kk["rstd_b"], q("norm.weight"))
            put(f"{layer}.norm.weight", dgain, (dnb * kk["xhat_b"]).abs().sum(0))
            put(f"{layer}.norm.bias", dbias, dnb.abs().sum(0))
            dg0.append(dz1 + dz)
        dh0 = torch.cat(dg0, 1) * _gelu_grad(h0)
        put("dense1.bias", dh0.sum(0), dh0.abs().sum(0))
        put("dense1.weight", dh0.T @ n0, dh0.abs().T @ n0.abs())
        dn0 = dh0 @ P["dense1.weight"]
        dx, dgain, dbias, _ = _ln64_bwd(dn0, xhat0, rstd0, P["norm.weight"])
        put("norm.weight", dgain, (dn0 * xhat0).abs().sum(0))
        put("norm.bias", dbias, dn0.abs().sum(0))
        _, _, _, mag = _ln64_bwd(dh0.abs() @ P["dense1.weight"].abs(), xhat0.abs(), rstd0, P["norm.weight"].abs())
        out["dx0"], S["dx0"] = (G + dx).reshape(x0.shape), float((G.abs() + mag).max())
    out["S"] = S
    return out


def _compose(x0, leaves):
    """The layer from oracle.oracle's own arithmetic (stage_forward's lines for it) in the dtype of its arguments -> y."""
    sd = {"L." + k: v for k, v in leaves.items()}
    t = F.gelu(oracle._lin(sd, "L.dense1", oracle._ln(sd, "L.norm", x0)))
    c = x0.shape[-1]
    u, v = t[..., :c], t[..., c:]
    u = oracle._gmlp_branch(sd, "L.grid_gmlp_layer", "grid_gating_unit", u, True)
    v = oracle._gmlp_branch(sd, "L.block_gmlp_layer", "block_gating_unit", v, False)
    return oracle._lin(sd, "L.dense2", torch.cat([u, v], dim=-1)) + x0


def autograd64(x0, p, g):
    """The same gradients from float64 autograd over the oracle's arithmetic -> dict GRADS."""
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    xx = x0.double().clone().requires_grad_()
    (_compose(xx, leaves) * g.double()).sum().backward()
    out = {"d:" + k: leaves[k].grad for k in PARAMS}
    out["dx0"] = xx.grad
    return out


def compose_f32(x0, p, g=None, want_dx0=True):
    """The float32 torch-op composition on the tensors' device (what tools/bench_gmlp_train.py times) -> (y, dict GRADS or None)."""
    leaves = {k: p[k].detach().clone().requires_grad_(g is not None) for k in PARAMS}
    xx = x0.detach().clone().requires_grad_(g is not None and want_dx0)
    y = _compose(xx, leaves)
    if g is None:
        return y, None
    y.backward(g)
    grads = {"d:" + k: leaves[k].grad for k in PARAMS}
    grads["dx0"] = xx.grad
    return y.detach(), grads


def params_of(sd, stage=4):
    """The 26 parameters of ``down<stage>``'s layer out of a detector state dict -> dict PARAMS."""
    return {k: sd[f"down{stage}.{_SD_LAYER}{k}"].detach().clone().float() for k in PARAMS}


# ---- seeded cases -------------------------------------------------------------------------------------------------------------
def sweep_params(seed, c=256):
    """General random parameters at width ``c``: gains around 1, small biases, dense weights ~ 1 / sqrt(fan-in), a full non-symmetric Wt."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k in PARAMS:
        leaf = k.rsplit(".", 2)[-2:]
        if leaf[0] == "norm":
            p[k] = 1 + 0.3 * torch.randn(c, generator=g) if leaf[1] == "weight" else 0.2 * torch.randn(c, generator=g)
        elif leaf[1] == "weight":
            shape = {"dense1": (2 * c, c), "dense": (64, 64), "dense2": (c, 2 * c if k == "dense2.weight" else c)}[leaf[0]]
            p[k] = torch.randn(shape, generator=g) / shape[1] ** 0.5
        else:
            n = {"dense1": 2 * c, "dense": 64, "dense2": c}[leaf[0]]
            p[k] = 0.2 * torch.randn(n, generator=g)
    return p, g


def sweep_case(shape, seed, device=None, c=256):
    """Seeded general float32 inputs for a shape at width ``c`` -> (x0, params, g = dy), on the CPU.  x0 >= 0 with a share of exact zeros, as the
    ReLU in front of the layer leaves it.  GELU has no kink: nothing to keep away from.  ``device``: where the case is moved to
    after it was drawn, on the CPU generator either way."""
    b, hc, wc = shape
    p, g = sweep_params(seed, c)
    x0 = (torch.randn((b, hc, wc, c), generator=g) * (0.5 + torch.rand((b, hc, wc, 1), generator=g)) + 0.3).clamp(min=0)
    dy = torch.randn(x0.shape, generator=g) / (b * hc * wc)
    return T.to_device((x0, p, dy), device)


def model_inputs():
    """Case ``model`` without its stored x0, dy: the layer of synth.synthetic_state_dict(0), the seeded image the recorder feeds to
    the reference's network (head_train_common.model_inputs), the seeded dlogits, and the parameters of the tail behind the layer
    -> (image, params, dlogits, (RCAB params, head params, running))."""
    from balf_amd.utils import synth
    image, hp, dlogits, running = H.model_inputs()
    sd = synth.synthetic_state_dict(0)
    return image, params_of(sd), dlogits, (R.params_of(sd), hp, running)


LAYOUT_SHAPE = (1, 16, 24)                  # regions of 2 x 3 pixels: both maps and the orientation of Wt each change the result
EDGES_SHAPE = (2, 8, 16)
EDGES_CONST_ROW = (1, 2, 5)                 # the pixel of x0 whose channels are all 0.5: var = 0, xhat = 0 exactly
EDGES_GATE0 = 37                            # the block map's token with a zero row of Wt and bt = -1: mix + 1 == 0 exactly
EDGES_GAIN0 = 5                             # the channel with gain 0 in the three LayerNorms of the grid branch
# width -> (channel of a dense1 output, bias): GELU saturated both ways, one pair in each half of the 2C outputs
EDGES_SAT = {256: ((3, 9.0), (4, -9.0), (300, 9.0), (301, -9.0)), 128: ((3, 9.0), (4, -9.0), (150, 9.0), (151, -9.0))}
# the grid branch's c half: dense1 weight 0 and this bias -> c = gelu(9) = 9 on every channel of every pixel, exactly so in float32 and
# in float64 (Phi(9) rounds to 1), and sums of up to C nines are exact in any order: the gating LayerNorm sees var = 0, xhat = 0
EDGES_C_BIAS = 9.0
RECORD_WHOLE = 1 << 12                      # a reference result with more elements than this is recorded on some rows only


def layout_inputs(c=256):
    return sweep_case(LAYOUT_SHAPE, 2718, c=c)


def edges_inputs(c=256):
    """Case ``edges`` at width ``c`` -> (x0, params, g = dy): the sweep's generator on EDGES_SHAPE with the edges named above."""
    x0, p, dy = sweep_case(EDGES_SHAPE, 4242, c=c)
    x0[EDGES_CONST_ROW] = 0.5
    gl, gu = BRANCHES[0]
    bl, bu = BRANCHES[1]
    p[f"{gl}.dense1.weight"][c:] = 0.0
    p[f"{gl}.dense1.bias"][c:] = EDGES_C_BIAS
    p[f"{bl}.{bu}.dense.weight"][EDGES_GATE0] = 0.0
    p[f"{bl}.{bu}.dense.bias"][EDGES_GATE0] = -1.0
    for k in (f"{gl}.norm.weight", f"{gl}.{gu}.norm.weight", "norm.weight"):
        p[k][EDGES_GAIN0] = 0.0
    for k in ("dense1.bias", f"{bl}.dense1.bias"):
        for ch, v in EDGES_SAT[c]:
            p[k][ch] = v
    return x0, p, dy


def regenerated_inputs_digest(name):
    return inputs_digest(*{"model": model_inputs, "layout": layout_inputs, "edges": edges_inputs}[name]())


def fixture_case(fx, name):
    """-> (x0, params, g = dy) of a fixture case, float32 on the CPU.  Case ``model`` stores x0 and the dy that the reference's
    own channel-attention block sent back."""
    if name == "model":
        return torch.from_numpy(fx["model.x0"]), model_inputs()[1], torch.from_numpy(fx["model.dy"])
    return layout_inputs() if name == "layout" else edges_inputs()


recorded_part = functools.partial(T.recorded_part, whole=RECORD_WHOLE, every=32)
recorded = functools.partial(T.recorded, part=recorded_part)


# ---- the float64 restatement of train_head with a TrainableMixerTail ----------------------------------------------------------
def train64(chunk, p, rp, hp, running, presentations, lr=1e-3):
    """As rcab_train_common.train64 with the layer in front: ``chunk`` a list of (x0 src, x0 dst, heat_src, heat_dst) CPU tensors,
    Adam over float64 copies of the 26 parameters ``p``, the block's ten ``rp`` and the head's six ``hp`` -> the per-presentation
    mean losses."""
    from tests import detector_loss_common as D
    leaves = {k: p[k].double().clone().requires_grad_() for k in PARAMS}
    rl = {k: rp[k].double().clone().requires_grad_() for k in R.PARAMS}
    hl = {k: hp[k].double().clone().requires_grad_() for k in H.PARAMS}
    rm, rv = running[0].double().clone(), running[1].double().clone()
    opt = torch.optim.Adam(list(leaves.values()) + list(rl.values()) + list(hl.values()), lr=lr)
    means = []
    for _ in range(presentations):
        losses = []
        for src, dst, heat_src, heat_dst in chunk:
            opt.zero_grad()
            total = 0.0
            for x0, heat in ((src, heat_src), (dst, heat_dst)):
                x0 = x0.double()
                y = _compose(x0, leaves)
                x2 = R._compose(y, (y + x0).detach(), rl)
                z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
                logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
                res = D.restate64(logits.detach(), heat.float(), None, None)
                logits.backward(torch.from_numpy(res["grad"]))
                total += float(res["loss"])
            opt.step()
            losses.append(total)
        means.append(float(np.mean(losses)))
    return means
