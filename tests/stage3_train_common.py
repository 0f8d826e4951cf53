"""Shared by tests/test_stage3_train_host.py, tests/test_stage3_train_gpu.py, tests/test_stage3_guard_gpu.py,
tests/golden/make_stage3_train_golden.py and tools/bench_stage3_train.py: the fixture stage3_train.npz and its cases at C = 128;
the 2 x 2 max-pool's reference and cases; the float64 restatement of the whole of stages 3-4 and the head, chained from the units'
restatements (rcab_train_common, gmlp_train_common and linrelu_train_common state them, at the width of their input); the same
through float64 autograd over torch's own ops; the float32 torch-op composition; and a Python restatement of the units' buffer
layouts."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import gmlp_train_common as Gc
from tests import head_train_common as H
from tests import linrelu_train_common as Lc
from tests import rcab_train_common as Rc
from tests import train_common as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage3_train.npz")
C3 = 128                                    # stage 3's width
TOL_FLOOR = H.TOL_FLOOR
KINK_FACTOR = 8.0                           # see assert_kink_margin
POOL_FACTOR = 8.0                           # two values of a 2 x 2 window lie at least this many float32 movements of pre apart
RCAB_PARAMS, RCAB_GRADS, RCAB_GATED = Rc.PARAMS, Rc.GRADS, Rc.GATED
GMLP_PARAMS, GMLP_GRADS, GMLP_GATED = Gc.PARAMS, Gc.GRADS, Gc.GATED
RCAB_CASES, GMLP_CASES = ("model", "edges"), ("model", "layout", "edges")
RCAB_SD = Rc.SD_NAMES
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
    return {3: ((sd["down3.conv.0.weight"].float(), sd["down3.conv.0.bias"].float()), Gc.params_of(sd, 3), Rc.params_of(sd, 3)),
            4: ((sd["down4.conv.0.weight"].float(), sd["down4.conv.0.bias"].float()), Gc.params_of(sd, 4), Rc.params_of(sd, 4)),
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
        gm = Gc.restate64(x0, gp)
        rc = Rc.restate64(gm["y"], gm["y"] + x0, rp)
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
        rc = Rc.restate64(y, y + x0, rp, g)
        gm = Gc.restate64(x0, gp, rc["dy"])
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
        y = Gc._compose(x0, gl)
        x = Rc._compose(y, (y + x0).detach(), rl) + (x0 - x0.detach())
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
    return Rc.edges_inputs(c=C3)


def gmlp_case(name):
    """-> (x0, params, g = dy) of a fixture case at C = 128; ``model`` as in rcab_case, from x0 and dy of case ``stage``."""
    if name == "model":
        res, sp = _stage_res(), stage_inputs(fixture())[1]
        return res["x0"].float(), sp[3][1], res["dy"].reshape(res["x0"].shape).float()
    return Gc.layout_inputs(c=C3) if name == "layout" else Gc.edges_inputs(c=C3)


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
