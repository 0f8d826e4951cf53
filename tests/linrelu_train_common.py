"""Shared by tests/test_linrelu_train_host.py, tests/test_linrelu_train_gpu.py, tests/golden/make_linrelu_train_golden.py and
tools/bench_stage4_train.py: the fixture linrelu_train.npz, the float64 restatement of the first layer of a Down stage (include/
balf_hip.h: balf_linrelu_train_forward, y = relu(x w^T + b) per pixel, c_out = 2 c_in) and of its backward as closed formulas, the
same through float64 autograd, the float32 torch-op composition, the error measure of the gates, the seeded case generators, and
the float64 restatement of train_head over all of stage 4."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import gmlp_train_common as G
from tests import head_train_common as H
from tests import rcab_train_common as R
from tests import train_common as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linrelu_train.npz")
FIXTURE_CASES = ("model", "edges", "c32", "c64")
PARAMS = ("weight", "bias")                 # = balf_amd.ops.LINRELU_PARAMS
GRADS = ("dw", "db", "dx")
GATED = ("y",) + GRADS
WIDTHS = (32, 64, 128)
TOL_FLOOR = H.TOL_FLOOR
# No pre-activation of a fixture case, except exact zeros, lies closer to the ReLU kink than KINK_FACTOR times the largest movement
# that float32 rounding gives to any element of y in that case (the recorder measures both on the reference's own float32 result
# and stores them), so a float32 implementation and the float64 restatement take the same mask; an element on the other side would
# be an error of a whole term, at any tolerance.
KINK_FACTOR = 8.0
SD_PREFIX = "down4.conv.0."
err = G.err


def fixture():
    return np.load(FIXTURE)


def restate64(x, w, b, g=None):
    """The equations of include/balf_hip.h in float64 on the CPU.  ``x`` [..., c_in], ``w`` [2 c_in, c_in], ``b`` [2 c_in]; ``g`` =
    the total gradient at y, or None.  -> dict of float64 tensors: h (the pre-activation), y, and with ``g``: gm, dw, db, dx; and
    ``S``: name -> the scale of the error measure, the largest sum of absolute values of the terms of that output's reduction (y:
    |x| |w|^T + |b|; db: sum_p |gm|; dw: |gm|^T |x|; dx: |gm| |w|).  The mask is h > 0 in float64: see KINK_FACTOR."""
    c_in = x.shape[-1]
    X = x.reshape(-1, c_in).double()
    W, B = w.double(), b.double()
    h = X @ W.T + B
    y = h.clamp(min=0)
    out = {"h": h, "y": y.reshape(tuple(x.shape[:-1]) + (2 * c_in,))}
    S = {"y": float((X.abs() @ W.abs().T + B.abs()).max())}
    if g is not None:
        G64 = g.reshape(-1, 2 * c_in).double()
        gm = torch.where(h > 0, G64, torch.zeros_like(G64))     # a select: whatever g holds under a dead unit gives 0
        out.update(gm=gm, db=gm.sum(0), dw=gm.T @ X, dx=(gm @ W).reshape(x.shape))
        S.update(db=float(gm.abs().sum(0).max()), dw=float((gm.abs().T @ X.abs()).max()), dx=float((gm.abs() @ W.abs()).max()))
    out["S"] = S
    return out


def autograd64(x, w, b, g):
    """The same gradients from float64 autograd over torch's own linear and relu -> dict GRADS."""
    xx, ww, bb = (t.double().clone().requires_grad_() for t in (x, w, b))
    (F.relu(F.linear(xx, ww, bb)) * g.double()).sum().backward()
    return {"dw": ww.grad, "db": bb.grad, "dx": xx.grad}


def compose_f32(x, w, b, g=None, want_dx=True):
    """The float32 torch-op composition on the tensors' device -> (y, dict GRADS or None)."""
    ww, bb = (t.detach().clone().requires_grad_(g is not None) for t in (w, b))
    xx = x.detach().clone().requires_grad_(g is not None and want_dx)
    y = F.relu(F.linear(xx, ww, bb))
    if g is None:
        return y, None
    y.backward(g)
    return y.detach(), {"dw": ww.grad, "db": bb.grad, "dx": xx.grad}


def kink_distance(res):
    """The smallest |pre-activation| that is not exactly zero."""
    return H.kink_distance(res["h"])


def params_of(sd):
    """``down4.conv.0`` out of a detector state dict -> (weight [256,128], bias [256])."""
    return tuple(sd[SD_PREFIX + k].detach().clone().float() for k in PARAMS)


# ---- seeded cases -------------------------------------------------------------------------------------------------------------
def sweep_case(n, c_in, seed, device=None):
    """Seeded inputs of the sweep -> (x [n, c_in], w, b, g [n, 2 c_in]), float32 on the CPU.  As head_train_common.sweep_case: x holds
    multiples of 1/8 in [-1, 1], w multiples of 1/16 in [-1/2, 1/2] and b odd multiples of 1/256, so every pre-activation is an odd
    multiple of 1/256 below 2^7, exact in float32 in any order and never closer than 1/256 to the kink; the mask of a float32
    implementation cannot differ from the restatement's.  g is general, with a sixteenth of exact zeros; dw, db and dx are general
    float32 sums.  The float32 rounding of the product itself is covered by the fixture cases, whose inputs are general.
    ``device``: where the case is moved to after it was drawn, on the CPU generator either way."""
    gen = torch.Generator().manual_seed(3000 + seed)
    x = torch.randint(-8, 9, (n, c_in), generator=gen).float() / 8
    w = torch.randint(-8, 9, (2 * c_in, c_in), generator=gen).float() / 16
    b = (2 * torch.randint(-64, 64, (2 * c_in,), generator=gen) + 1).float() / 256
    g = torch.randn((n, 2 * c_in), generator=gen) / n
    g[torch.rand((n, 2 * c_in), generator=gen) < 1 / 16] = 0.0
    return T.to_device((x, w, b, g), device)


def keypoint_map():
    """The seeded labels of case ``model`` [2,1,64,64]: at most one keypoint in a cell of 8 x 8 pixels, in about half of the cells,
    so the reference's loss has no tie to break and its random tie-break noise cannot change the labels."""
    rng = np.random.Generator(np.random.PCG64([2024, 3]))
    heat = np.zeros((2, 1, 64, 64), np.float32)
    for b in range(2):
        for cy in range(8):
            for cx in range(8):
                if rng.random() < 0.5:
                    heat[b, 0, 8 * cy + rng.integers(8), 8 * cx + rng.integers(8)] = 1.0
    return torch.from_numpy(heat)


def model_inputs():
    """Case ``model`` without what the fixture stores (x3, the gradient at x0, dlogits): ``down4.conv.0`` of
    synth.synthetic_state_dict(0), the seeded image that the recorder feeds to the reference's network, and the labels of the
    reference's loss -> (image, (weight, bias), keypoint map)."""
    from balf_amd.utils import synth
    image = H.model_inputs()[0]
    return image, params_of(synth.synthetic_state_dict(0)), keypoint_map()


EDGES_N = 37                                # an odd count: partial tiles everywhere
EDGES_ZERO_ROW = 5                          # x[5] = 0: with b = 0 on channels 0..7, h == 0 exactly there, in either precision
EDGES_DEAD = 100                            # the channel with a zero row of w and b = -9: dead on every pixel
EDGES_BIAS = ((100, -9.0), (101, 9.0), (200, -9.0), (201, 9.0))     # (channel, bias); 200 keeps its row of w: dead all the same
EDGES_HUGE = 1e30                           # g under the dead channels 100 and 200


def edges_inputs():
    """Case ``edges`` at c_in = 128 -> (x [37,128], w, b, g [37,256]): general seeded values with the edges named above."""
    gen = torch.Generator().manual_seed(5151)
    x = torch.randn((EDGES_N, 128), generator=gen) * 0.5
    w = torch.randn((256, 128), generator=gen) / 128 ** 0.5
    b = 0.2 * torch.randn((256,), generator=gen)
    g = torch.randn((EDGES_N, 256), generator=gen) / EDGES_N
    x[EDGES_ZERO_ROW] = 0.0
    b[:8] = 0.0
    g[EDGES_ZERO_ROW, :8] = torch.arange(1, 9).float()          # a non-zero g on the exact zeros
    w[EDGES_DEAD] = 0.0
    for c, v in EDGES_BIAS:
        b[c] = v
    g[:, EDGES_DEAD] = EDGES_HUGE
    g[:, 200] = -EDGES_HUGE
    return x, w, b, g


def width_inputs(c_in):
    """Cases ``c32`` and ``c64`` -> (x [N, c_in], w, b, g): general seeded values in the layout of nn.Linear(c_in, 2 c_in); N = 70 and
    131, no multiple of a tile."""
    n = {32: 70, 64: 131}[c_in]
    gen = torch.Generator().manual_seed(6000 + c_in)
    x = torch.randn((n, c_in), generator=gen) * (0.5 + torch.rand((n, 1), generator=gen))
    w = torch.randn((2 * c_in, c_in), generator=gen) / c_in ** 0.5
    b = 0.3 * torch.randn((2 * c_in,), generator=gen)
    g = torch.randn((n, 2 * c_in), generator=gen) / n
    return x, w, b, g


def _flat(case):
    out = []
    for t in case:
        out.extend(t if isinstance(t, (tuple, list)) else (t,))
    return tuple(out)


def regenerated_inputs_digest(name):
    """SHA-256 of everything of case ``name`` that the fixture does not store (train_common.inputs_digest)."""
    case = {"model": model_inputs, "edges": edges_inputs, "c32": lambda: width_inputs(32), "c64": lambda: width_inputs(64)}[name]()
    return T.inputs_digest(*_flat(case))


def fixture_case(fx, name):
    """-> (x, w, b, g) of a fixture case, float32 on the CPU.  Case ``model`` stores x3 and the total gradient at x0 that the
    reference's stage 4 sent back under the reference's loss."""
    if name == "model":
        w, b = model_inputs()[1]
        return torch.from_numpy(fx["model.x"]), w, b, torch.from_numpy(fx["model.g"])
    return edges_inputs() if name == "edges" else width_inputs(int(name[1:]))


# ---- the float64 restatement of train_head with a TrainableStage4 ---------------------------------------------------------------
def stage4_compose(x3, w0, b0, gl, rl):
    """x3 -> x2 of down4 in the dtype of its arguments: conv.0 and its ReLU, the gated-MLP layer (gmlp_train_common._compose), the
    channel-attention block (rcab_train_common._compose, which holds the long shortcut constant) and the long shortcut's own
    gradient, added as an exact zero."""
    x0 = F.relu(F.linear(x3, w0, b0))
    y = G._compose(x0, gl)
    return R._compose(y, (y + x0).detach(), rl) + (x0 - x0.detach())


def train64(chunk, conv0, p, rp, hp, running, presentations, lr=1e-3):
    """As gmlp_train_common.train64 with ``down4.conv.0`` in front: ``chunk`` a list of (x3 src, x3 dst, heat_src, heat_dst) CPU
    tensors, Adam over float64 copies of ``conv0`` = (weight, bias), the layer's 26 ``p``, the block's ten ``rp`` and the head's six
    ``hp``, in the order of TrainableStage4.parameters() -> the per-presentation mean losses."""
    from tests import detector_loss_common as D
    w0, b0 = (t.double().clone().requires_grad_() for t in conv0)
    leaves = {k: p[k].double().clone().requires_grad_() for k in G.PARAMS}
    rl = {k: rp[k].double().clone().requires_grad_() for k in R.PARAMS}
    hl = {k: hp[k].double().clone().requires_grad_() for k in H.PARAMS}
    rm, rv = running[0].double().clone(), running[1].double().clone()
    opt = torch.optim.Adam([w0, b0] + list(leaves.values()) + list(rl.values()) + list(hl.values()), lr=lr)
    means = []
    for _ in range(presentations):
        losses = []
        for src, dst, heat_src, heat_dst in chunk:
            opt.zero_grad()
            total = 0.0
            for x3, heat in ((src, heat_src), (dst, heat_dst)):
                x2 = stage4_compose(x3.double(), w0, b0, leaves, rl)
                z = F.linear(F.relu(F.linear(x2, hl["w2"], hl["b2"])), hl["wd"], hl["bd"]).permute(0, 3, 1, 2)
                logits = F.batch_norm(z, rm, rv, hl["gamma"], hl["beta"], training=True, momentum=H.MOMENTUM, eps=H.EPS)
                res = D.restate64(logits.detach(), heat.float(), None, None)
                logits.backward(torch.from_numpy(res["grad"]))
                total += float(res["loss"])
            opt.step()
            losses.append(total)
        means.append(float(np.mean(losses)))
    return means
