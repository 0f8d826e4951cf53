#!/usr/bin/env python3
"""Record tests/golden/stage3_train.npz from the REFERENCE's own modules and PyTorch's autograd on the CPU.

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    python tests/golden/make_stage3_train_golden.py

Case ``stage``: the reference's MLP_MA_DECODER with synth.synthetic_state_dict(0) in .train() on the seeded 2 x 3 x 64 x 64 image
of tests/head_train_common.py: model_inputs, under the reference's own detector_loss on the labels of
linrelu_train_common.keypoint_map.  A forward-pre-hook captures x2s at down3.conv (the stage-2 output: the map of stage 3 is
16 x 16 and that of stage 4 8 x 8), forward hooks the pre-activation of every ReLU / LeakyReLU of stages 3-4 and the input of the
pool.  Stored: x2s and dlogits (the inputs), the reference's float32 gradients of the 38 tensors of down3 and x2s.grad.  Asserted
and stored: the kink margin of stage3_train_common.assert_kink_margin on every one of them (the reference's masks are the
restatement's); the two largest values of every 2 x 2 window of ``pre`` lie POOL_FACTOR float32 movements of pre apart and the
reference's pooled map is the restatement's choice.

Unit cases at C = 128, through the reference's ResidualChannelAttentionBlock(128) and ResidualSplitHeadMultiAxisGmlpLayer(128,
(8, 8), (8, 8)) constructed on their own: ``model`` (stage3_train_common.rcab_case / gmlp_case: the units' inputs inside case
``stage``, with the weights of down3), ``edges`` and, for the layer, ``layout``.  nn.MaxPool2d(2) is torch's max_pool2d, which the
pool's tests call directly and match bit for bit: nothing to record.

Gates: d_T = the largest err (against the float64 restatement at width C) of the reference's own float32 result over a unit's
cases, stored as <unit>.d_<T>; the tests take tol_T = max(4 * d_T, 1.1e-6).  Large results are recorded on some rows only
(stage3_train_common.recorded_part).  Nothing of the reference is committed: the fixture holds numbers only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import ref_model                                      # noqa: E402  (puts the reference on the path)
from tests.golden.make_linrelu_train_golden import reference_loss                    # noqa: E402
from balf.model.mlp_ma_decoder import ResidualChannelAttentionBlock, ResidualSplitHeadMultiAxisGmlpLayer   # noqa: E402  (reference)
from tests import gmlp_train_common as Gc                                           # noqa: E402
from tests import head_train_common as H                                            # noqa: E402
from tests import linrelu_train_common as Lc                                        # noqa: E402
from tests import rcab_train_common as Rc                                           # noqa: E402
from tests import stage3_train_common as Sc                                         # noqa: E402


def run_stage_case():
    image = H.model_inputs()[0]
    m, _ = ref_model(0)
    m.train()
    seen = {}

    def keep_input(name):
        def hook(_module, args):
            args[0].retain_grad()
            seen[name] = args[0]
        return hook

    def keep_output(name):
        def hook(_module, _args, out):
            seen[name] = out.detach().clone()               # (before an in-place ReLU behind it)
        return hook

    handles = [m.down3.conv.register_forward_pre_hook(keep_input("x2s")),
               m.down3.conv_down.register_forward_pre_hook(keep_input("pre"))]
    for s, down in ((3, m.down3), (4, m.down4)):
        rcab = down.residual_channel_attention_block
        handles += [down.conv[0].register_forward_hook(keep_output(f"down{s}.conv.0")),
                    rcab.conv1.register_forward_hook(keep_output(f"down{s}.rcab.conv1")),
                    rcab.calayer.excite[0].register_forward_hook(keep_output(f"down{s}.rcab.excite.0"))]
    handles.append(m.down4.conv2.register_forward_hook(keep_output("down4.conv2")))
    out = m(image)
    for h in handles:
        h.remove()
    logits = out["logits"]
    logits.retain_grad()
    torch.manual_seed(0)                                        # the tie-break noise, which these labels leave without effect
    reference_loss()(Lc.keypoint_map(), logits).backward()
    x2s = seen["x2s"]
    own = dict(m.down3.named_parameters())
    got = {"d:" + n: own[n].grad for n in Sc.STAGE3_NAMES}
    got["dx2s"] = x2s.grad
    return x2s.detach().contiguous(), logits.grad.contiguous(), got, seen, m.down3.conv_down(seen["pre"].detach())


def run_rcab_case(name):
    y, r, p, g = Sc.rcab_case(name)
    block = ResidualChannelAttentionBlock(Sc.C3).train()
    own = dict(block.named_parameters())
    with torch.no_grad():
        for k, n in Sc.RCAB_SD.items():
            own[n].copy_(p[k])
    seen = {}
    handles = [block.conv1.register_forward_hook(lambda _m, _a, out: seen.update(h=out.detach().clone())),
               block.calayer.excite[0].register_forward_hook(lambda _m, _a, out: seen.update(se_pre=out.detach().clone()))]
    yy = y.clone().requires_grad_()
    x2 = block(yy) + (r - y)                                    # Down.forward adds the long shortcut behind the block
    for h in handles:
        h.remove()
    x2.backward(g)
    return (y, r, p, g), dict({"d" + k: own[n].grad for k, n in Sc.RCAB_SD.items()}, x2=x2.detach(), dy=yy.grad), seen


def run_gmlp_case(name):
    x0, p, g = Sc.gmlp_case(name)
    layer = ResidualSplitHeadMultiAxisGmlpLayer(Sc.C3, (8, 8), (8, 8)).train()
    own = dict(layer.named_parameters())
    with torch.no_grad():
        for k in Sc.GMLP_PARAMS:
            own[k].copy_(p[k])
    xx = x0.clone().requires_grad_()
    y = layer(xx)
    y.backward(g)
    return (x0, p, g), dict({"d:" + k: own[k].grad for k in Sc.GMLP_PARAMS}, y=y.detach(), dx0=xx.grad), {}


def record(fx, unit, name, got, res, gated, d):
    line = []
    for k in gated:
        e = Sc.err(got[k], res[k], res["S"][k])
        assert np.isfinite(e), (unit, name, k)
        d[k] = max(d.get(k, 0.0), e)
        line.append(f"{k.rsplit('.', 2)[-2][:6] + '.' + k.rsplit('.', 1)[-1][:1] if '.' in k else k} {e:.1e}")
        fx[f"{unit}.{name}.{k}"] = Sc.recorded_part(got[k].detach()).contiguous().numpy().astype(np.float32)
    print(f"{unit} {name}: " + " ".join(line))


def main():
    torch.manual_seed(0)
    fx = {}
    # ---- the whole stage first: the unit cases ``model`` are cut out of it
    x2s, dlogits, got, seen, pooled = run_stage_case()
    fx["stage.x2s"], fx["stage.dlogits"] = x2s.numpy(), dlogits.numpy()
    np.savez_compressed(Sc.FIXTURE, **fx)                       # (stage_inputs and the unit cases read the file)
    x2s_, sp, dlogits_ = Sc.stage_inputs(Sc.fixture())
    res = Sc.stage64(x2s_, sp, dlogits_)
    ag = Sc.stage_autograd64(x2s_, sp, dlogits_)
    for k in Sc.STAGE_GATED:
        assert Sc.err(ag[k], res[k], res["S"][k]) <= 1e-12, ("stage", k, Sc.err(ag[k], res[k], res["S"][k]))
    d = {}
    record(fx, "stage", "model", got, res, Sc.STAGE_GATED, d)
    for k in Sc.STAGE_GATED:
        fx[f"stage.d_{k}"] = np.float64(d[k])
    print("stage: largest d_T", max(d.values()), "tol", max(4 * max(d.values()), Sc.TOL_FLOOR))
    for name, h64 in res["kinks"].items():
        h32 = seen[name].double().reshape(h64.shape)
        kink, moved = H.kink_distance(h64), float((h32 - h64).abs().max())
        print(f"kink {name}: nearest {kink:.2e}, float32 movement {moved:.2e}")
        Sc.assert_kink_margin(h32, h64, name)
        fx[f"stage.kink.{name}"], fx[f"stage.moved.{name}"] = np.float64(kink), np.float64(moved)
    pre32 = seen["pre"].detach().permute(0, 2, 3, 1).double()
    moved = float((pre32 - res["pre"]).abs().max())
    print(f"pool: smallest gap of a window {res['pool_gap']:.2e}, float32 movement of pre {moved:.2e}")
    assert res["pool_gap"] > Sc.POOL_FACTOR * moved
    want, which, _ = Sc.pool_reference(pre32.float())
    assert torch.equal(pooled.permute(0, 2, 3, 1), want)
    assert torch.equal(which, Sc.pool_reference(res["pre"])[1])        # the reference's float32 choice is the restatement's
    fx["stage.pool_gap"], fx["stage.pool_moved"] = np.float64(res["pool_gap"]), np.float64(moved)
    # ---- the units at C = 128
    for unit, cases, run, restate, autograd, gated, grads in (
            ("rcab", Sc.RCAB_CASES, run_rcab_case, Rc.restate64, Rc.autograd64, Sc.RCAB_GATED, Sc.RCAB_GRADS),
            ("gmlp", Sc.GMLP_CASES, run_gmlp_case, Gc.restate64, Gc.autograd64, Sc.GMLP_GATED, Sc.GMLP_GRADS)):
        d = {}
        for name in cases:
            inputs, got, seen = run(name)
            res, ag = restate(*inputs), autograd(*inputs)
            for k in grads:
                assert Sc.err(ag[k], res[k], res["S"][k]) <= 1e-12, (unit, name, k)
            record(fx, unit, name, got, res, gated, d)
            fx[f"{unit}.{name}.inputs_sha256"] = np.asarray(Sc.T.inputs_digest(*inputs))
            for k, h32 in seen.items():                         # the LeakyReLU and the squeeze-excite ReLU
                h32 = h32.double().reshape(res[k].shape)
                kink, moved = H.kink_distance(res[k]), float((h32 - res[k]).abs().max())
                print(f"rcab {name}: {k} nearest {kink:.2e}, float32 movement {moved:.2e}")
                Sc.assert_kink_margin(h32, res[k], (name, k))
                fx[f"rcab.{name}.kink.{k}"], fx[f"rcab.{name}.moved.{k}"] = np.float64(kink), np.float64(moved)
        for k in gated:
            fx[f"{unit}.d_{k}"] = np.float64(d[k])
            print(f"{unit}.d_{k} {d[k]:.3e} tol {max(4 * d[k], Sc.TOL_FLOOR):.3e}")
    np.savez_compressed(Sc.FIXTURE, **fx)
    print("wrote", Sc.FIXTURE, os.path.getsize(Sc.FIXTURE), "bytes")
    assert os.path.getsize(Sc.FIXTURE) < 1000000


if __name__ == "__main__":
    main()
