"""What stage 3's training adds, without a GPU: balf_train_unit_sizes against the existing size queries and against a Python
restatement of the layouts, its error codes, the ops' argument checks at channels=128, the parameter shapes and counts,
TrainableStage3's state handling, the units' float64 restatements at C = 128 and that of the stage (tests/stage3_train_common.py)
against float64 autograd over torch's own ops, and the fixture against the restatements."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.model import get_model
from balf_amd.model.stage3_train import TrainableStage3
from balf_amd.utils import synth
from tests import gmlp_train_common as G
from tests import rcab_train_common as R
from tests import stage3_train_common as Sc
from tests import train_common as T
from tests.test_workspace_bytes_host import TABLE

OK, ERR_ARG, ERR_SHAPE = 0, -1, -2
C3 = Sc.C3
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return Sc.fixture()


def sizes(lib, unit, c, b, h, w):
    """-> (return code, workspace bytes, saved bytes); the outputs start at SENTINEL."""
    ws, sv = C.c_size_t(SENTINEL), C.c_size_t(SENTINEL)
    rc = lib.balf_train_unit_sizes(unit, c, b, h, w, C.byref(ws), C.byref(sv))
    return rc, ws.value, sv.value


# ---- balf_train_unit_sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,name", ((_lib.UNIT_RCAB, "rcab"), (_lib.UNIT_GMLP, "gmlp")))
def test_unit_sizes_at_256_are_the_existing_queries(lib, unit, name):
    """Over the argument tables of tests/test_workspace_bytes_host.py, the invalid set included (there the queries return 0 and
    this one a code, the outputs untouched)."""
    valid, invalid = TABLE[f"balf_{name}_train_workspace_bytes"]
    assert (valid, invalid) == TABLE[f"balf_{name}_train_saved_bytes"]
    ws_q, sv_q = getattr(lib, f"balf_{name}_train_workspace_bytes"), getattr(lib, f"balf_{name}_train_saved_bytes")
    for dims in valid:
        assert sizes(lib, unit, 256, *dims) == (OK, ws_q(*dims), sv_q(*dims)), dims
    assert ws_q(*invalid) == 0 and sv_q(*invalid) == 0
    rc, ws, sv = sizes(lib, unit, 256, *invalid)
    assert rc in (ERR_ARG, ERR_SHAPE) and (ws, sv) == (SENTINEL, SENTINEL)


@pytest.mark.parametrize("c", (128, 256))
def test_unit_sizes_equal_the_restated_layout(lib, c):
    for dims in ((1, 1, 2), (2, 1, 1), (3, 3, 5), (63, 1, 5), (1, 129, 131), (2, 257, 257), (16, 64, 80)):
        assert sizes(lib, _lib.UNIT_RCAB, c, *dims) == (OK,) + Sc.unit_sizes("rcab", c, *dims), dims
    for dims in ((1, 8, 8), (2, 8, 16), (3, 16, 24), (1, 24, 40), (1, 8, 2056), (2, 216, 152), (16, 64, 80)):
        assert sizes(lib, _lib.UNIT_GMLP, c, *dims) == (OK,) + Sc.unit_sizes("gmlp", c, *dims), dims
    for dims in ((1, 2, 2), (3, 6, 10), (2, 16, 16), (16, 128, 160)):
        for cc in (4, 32, c):
            assert sizes(lib, _lib.UNIT_POOL, cc, *dims) == (OK,) + Sc.unit_sizes("pool", cc, *dims), (dims, cc)


def test_unit_sizes_error_codes_leave_the_outputs_alone(lib):
    untouched = (SENTINEL, SENTINEL)
    for unit in (-1, 3, 99):
        assert sizes(lib, unit, 128, 1, 8, 8) == (ERR_ARG,) + untouched
    for unit in (_lib.UNIT_RCAB, _lib.UNIT_GMLP):
        for c in (0, 64, 127, 192, 512, -128):
            assert sizes(lib, unit, c, 1, 8, 8) == (ERR_SHAPE,) + untouched, (unit, c)
        for dims in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -8)):
            assert sizes(lib, unit, 128, *dims) == (ERR_ARG,) + untouched, (unit, dims)
        assert sizes(lib, unit, 128, 2, 4096, 4096) == (ERR_SHAPE,) + untouched                # N > 2^24
    assert sizes(lib, _lib.UNIT_RCAB, 128, 1, 1, 1) == (ERR_ARG,) + untouched                      # one value per channel
    for dims in ((1, 7, 8), (1, 8, 12)):
        assert sizes(lib, _lib.UNIT_GMLP, 128, *dims) == (ERR_SHAPE,) + untouched                  # no multiple of 8
    for dims in ((1, 3, 4), (1, 4, 5), (2, 1, 1)):
        assert sizes(lib, _lib.UNIT_POOL, 128, *dims) == (ERR_SHAPE,) + untouched                  # an odd input map
    for c in (0, 2, 6, 260):
        assert sizes(lib, _lib.UNIT_POOL, c, 1, 4, 4) == (ERR_SHAPE,) + untouched
    assert sizes(lib, _lib.UNIT_POOL, 128, 0, 4, 4) == (ERR_ARG,) + untouched
    assert sizes(lib, _lib.UNIT_POOL, 128, 1, 4096, 4098) == (ERR_SHAPE,) + untouched
    ws = C.c_size_t(SENTINEL)
    assert lib.balf_train_unit_sizes(_lib.UNIT_POOL, 128, 1, 4, 4, None, C.byref(ws)) == ERR_ARG and ws.value == SENTINEL
    assert lib.balf_train_unit_sizes(_lib.UNIT_POOL, 128, 1, 4, 4, C.byref(ws), None) == ERR_ARG and ws.value == SENTINEL
    with pytest.raises(_lib.BalfHipError, match="balf_train_unit_sizes"):
        ops.train_unit_sizes(_lib.UNIT_GMLP, 128, 1, 7, 8)


def test_entry_points_refuse_a_bad_width_before_anything_else(lib):
    """C other than 128 or 256: BALF_ERR_SHAPE, whatever the other arguments are (all NULL here), and the pool's own checks."""
    for c in (0, 64, 192, 512):
        assert lib.balf_rcab_train_forward_c(*([None] * 12), 1, 8, 8, c, None, None, None, 0, None) == ERR_SHAPE
        assert lib.balf_rcab_train_backward_c(*([None] * 8), 1, 8, 8, c, *([None] * 12), 0, None) == ERR_SHAPE
        assert lib.balf_gmlp_train_forward_c(None, None, 1, 8, 8, c, None, None, None, 0, None) == ERR_SHAPE
        assert lib.balf_gmlp_train_backward_c(None, None, None, None, 1, 8, 8, c, None, None, None, 0, None) == ERR_SHAPE
    for c in (128, 256):                                            # a good width reaches the pointer checks
        assert lib.balf_rcab_train_forward_c(*([None] * 12), 1, 8, 8, c, None, None, None, 0, None) == ERR_ARG
        assert lib.balf_gmlp_train_forward_c(None, None, 1, 8, 8, c, None, None, None, 0, None) == ERR_ARG
    fake = C.c_void_p(4096)
    assert lib.balf_pool_train_forward(None, 1, 4, 4, 8, fake, fake, None) == ERR_ARG
    assert lib.balf_pool_train_forward(fake, 1, 3, 4, 8, fake, fake, None) == ERR_SHAPE
    assert lib.balf_pool_train_forward(C.c_void_p(4100), 1, 4, 4, 8, fake, fake, None) == ERR_ARG
    assert lib.balf_pool_train_backward(fake, fake, 1, 4, 5, 8, fake, None) == ERR_SHAPE
    assert lib.balf_pool_train_backward(fake, C.c_void_p(4104), 1, 4, 4, 8, fake, None) == ERR_ARG


# ---- ops ---------------------------------------------------------------------------------------------------------------------------
def test_param_shapes_and_counts():
    assert ops.rcab_param_shapes(256) is ops._RCAB_PARAM_SHAPES and ops.gmlp_param_shapes(256) is ops._GMLP_PARAM_SHAPES
    assert ops.rcab_param_shapes() is ops._RCAB_PARAM_SHAPES and ops.gmlp_param_shapes() is ops._GMLP_PARAM_SHAPES
    r, g = ops.rcab_param_shapes(128), ops.gmlp_param_shapes(128)
    assert tuple(r) == ops.RCAB_PARAMS and tuple(g) == ops.GMLP_PARAMS
    assert r["ws0"] == (32, 128) and r["ws2"] == (128, 32) and r["wc1"] == (128, 128) and r["bs0"] == (32,)
    assert g["dense1.weight"] == (256, 128) and g["dense2.weight"] == (128, 256)
    assert g["grid_gmlp_layer.grid_gating_unit.dense.weight"] == (64, 64) and g["block_gmlp_layer.dense2.weight"] == (128, 128)
    count = lambda shapes: sum(int(np.prod(s)) for s in shapes.values())                 # noqa: E731
    assert count(r) == 41632 and count(g) == 174592 and count(r) + count(g) + 128 * 64 + 128 == 224544
    sd = synth.synthetic_state_dict(0)
    for k, shape in g.items():
        assert tuple(sd["down3.residual_split_head_multi_axis_gmlp_layer." + k].shape) == shape, k
    for k, shape in r.items():
        assert tuple(sd["down3.residual_channel_attention_block." + Sc.RCAB_SD[k]].shape) == shape, k
    for bad in (64, 0, 512, None):
        with pytest.raises(_lib.BalfHipError, match="channels must be one of"):
            ops.rcab_param_shapes(bad)
        with pytest.raises(_lib.BalfHipError, match="channels must be one of"):
            ops.gmlp_param_shapes(bad)


def test_ops_argument_errors_at_128():
    y, r, p, g = R.sweep_case((1, 2, 3), 1, c=C3)
    params = [p[k] for k in R.PARAMS]
    with pytest.raises(_lib.BalfHipError, match="GPU"):                      # right in every respect but the device
        ops.rcab_train_forward(y, r, params, channels=128)
    with pytest.raises(_lib.BalfHipError, match="\\[B,Hc,Wc,256\\].*stage 4"):   # the width is stated, never taken from y
        ops.rcab_train_forward(y, r, params)
    with pytest.raises(_lib.BalfHipError, match="\\[B,Hc,Wc,128\\].*stage 3"):
        ops.rcab_train_forward(torch.zeros(1, 2, 3, 256), r, params, channels=128)
    with pytest.raises(_lib.BalfHipError, match="channels must be one of"):
        ops.rcab_train_forward(y, r, params, channels=64)
    with pytest.raises(_lib.BalfHipError, match="ws0 must be \\[32, 128\\]"):
        ops.rcab_train_forward(y, r, params[:6] + [torch.zeros(64, 128)] + params[7:], channels=128)
    with pytest.raises(_lib.BalfHipError, match="r must be"):
        ops.rcab_train_forward(y, r[:, :1].contiguous(), params, channels=128)
    with pytest.raises(_lib.BalfHipError, match="wc1 must be \\[128, 128\\]"):
        ops.rcab_train_backward(g, y, p["ln_g"], torch.zeros(256, 256), p["wc2"], p["ws0"], p["ws2"], torch.zeros(8, dtype=torch.uint8),
                                channels=128)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.rcab_train_backward(g, y, p["ln_g"], p["wc1"], p["wc2"], p["ws0"], p["ws2"], torch.zeros(8, dtype=torch.uint8), channels=128)
    x0, gp, dy = G.sweep_case((1, 8, 8), 2, c=C3)
    gparams = [gp[k] for k in G.PARAMS]
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.gmlp_train_forward(x0, gparams, channels=128)
    with pytest.raises(_lib.BalfHipError, match="\\[B,Hc,Wc,256\\].*stage 4"):
        ops.gmlp_train_forward(x0, gparams)
    with pytest.raises(_lib.BalfHipError, match="\\[B,Hc,Wc,128\\].*stage 3"):
        ops.gmlp_train_forward(torch.zeros(1, 8, 8, 256), gparams, channels=128)
    with pytest.raises(_lib.BalfHipError, match="multiples of 8"):
        ops.gmlp_train_forward(torch.zeros(1, 8, 12, 128), gparams, channels=128)
    with pytest.raises(_lib.BalfHipError, match="dense1.weight must be \\[256, 128\\]"):
        ops.gmlp_train_forward(x0, gparams[:2] + [torch.zeros(512, 256)] + gparams[3:], channels=128)
    with pytest.raises(_lib.BalfHipError, match="dy must be"):
        ops.gmlp_train_backward(dy[:, :4].contiguous(), x0, gparams, torch.zeros(8, dtype=torch.uint8), channels=128)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.pool_train_forward(torch.zeros(1, 4, 4, 8))
    with pytest.raises(_lib.BalfHipError, match="multiple of 4"):
        ops.pool_train_forward(torch.zeros(1, 4, 4, 6))
    with pytest.raises(_lib.BalfHipError, match="multiple of 4"):
        ops.pool_train_forward(torch.zeros(4, 4, 8))
    with pytest.raises(_lib.BalfHipError, match="x must be float32"):
        ops.pool_train_forward(torch.zeros(1, 4, 4, 8).double())
    with pytest.raises(_lib.BalfHipError, match="even"):
        ops.pool_train_forward(torch.zeros(1, 4, 5, 8))
    with pytest.raises(_lib.BalfHipError, match="which must be"):
        ops.pool_train_backward(torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 4, dtype=torch.uint8))
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.pool_train_backward(torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 8, dtype=torch.uint8))
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    with pytest.raises(_lib.BalfHipError, match="CPU"):
        model.encode(torch.zeros(1, 3, 64, 64), level="stage2")
    stage = TrainableStage3()
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        stage(torch.zeros(1, 16, 16, 64))
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        stage.eval()(torch.zeros(1, 16, 16, 64))


# ---- TrainableStage3 -------------------------------------------------------------------------------------------------------------
def test_trainable_stage3_state():
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    sd = synth.synthetic_state_dict(2)
    model.load_state_dict(sd)
    stage = TrainableStage3.from_model(model)
    assert stage.training and stage.stage4.training and stage.stage4.mixer.tail.head.training and stage.encode_level == "stage2"
    state = stage.state_dict()
    assert tuple(state)[:38] == tuple("down3." + n for n in Sc.STAGE3_NAMES) == tuple("down3." + n for n in stage.stage3_names())
    assert list(state)[38:] == ["stage4." + k for k in stage.stage4.state_dict()]
    params = list(stage.parameters())
    own = list(stage.down3.parameters())
    assert len(own) == 38 and len(params) == 82
    assert sum(q.numel() for q in own) == 224544 and sum(q.numel() for q in params) == 1173923
    assert [tuple(q.shape) for q in stage.conv0_parameters()] == [(128, 64), (128,)]
    assert [tuple(q.shape) for q in stage.gmlp_parameters()] == list(ops.gmlp_param_shapes(128).values())
    assert [tuple(q.shape) for q in stage.rcab_parameters()] == list(ops.rcab_param_shapes(128).values())
    live = model.state_dict()
    for n, mine in stage.down3.named_parameters():
        assert torch.equal(mine, sd["down3." + n]) and mine.data_ptr() != live["down3." + n].data_ptr(), n
    key = model._weights_key("cpu")
    with torch.no_grad():                                                # what an optimiser step does to the copies
        for q in stage.parameters():
            q.add_(1.0)
    assert model._weights_key("cpu") == key
    assert torch.equal(model.state_dict()["down3.conv.0.weight"], sd["down3.conv.0.weight"])
    stage.commit(model)
    assert model._weights_key("cpu") != key
    after = model.state_dict()
    for n in Sc.STAGE3_NAMES:
        assert torch.equal(after["down3." + n], sd["down3." + n] + 1.0), n
    for k in ("down4.conv.0.weight", G.SD_PREFIX + "dense1.weight", "down4.conv2.weight", "detector_head.dense.bias"):
        assert torch.equal(after[k], sd[k] + 1.0), k
    for k in after:
        if k.startswith(("down1.", "down2.", "down3.conv2.")):
            assert torch.equal(after[k], sd[k]), k                       # stages 1-2 (and down3's unused conv2) stay frozen
    stage.eval()
    assert not stage.stage4.training and not stage.stage4.mixer.tail.head.training
    stage.train()
    assert stage.stage4.mixer.tail.head.training
    model.down3.residual_channel_attention_block.norm.eps = 1e-6
    with pytest.raises(ValueError, match="eps"):
        TrainableStage3.from_model(model)


# ---- the restatements and the fixture ------------------------------------------------------------------------------------------
def test_restatements_at_128_against_autograd():
    y, r, p, g = R.sweep_case((2, 3, 5), 3, c=C3)
    res, ag = R.restate64(y, r, p, g), R.autograd64(y, r, p, g)
    assert all(Sc.err(ag[k], res[k], res["S"][k]) <= 1e-12 for k in R.GRADS)
    x0, gp, dy = G.sweep_case(G.LAYOUT_SHAPE, 4, c=C3)
    res, ag = G.restate64(x0, gp, dy), G.autograd64(x0, gp, dy)
    assert all(Sc.err(ag[k], res[k], res["S"][k]) <= 1e-12 for k in G.GRADS)
    # the width is the input's: the stage's own copies of these restatements are gone, and the one statement serves both widths
    assert res["y"].shape[-1] == C3 and R.restate64(*R.sweep_case((1, 2, 3), 5))["x2"].shape[-1] == 256


def test_pool_reference_rule():
    """The rule the kernel states, on torch's own max_pool2d: first maximum, first of +0 / -0, last NaN."""
    nan = float("nan")
    x = torch.tensor([[1.0, 1.0, 1.0, 1.0], [0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, 0.0, 0.0], [nan, 2.0, nan, 1.0], [1.0, nan, 3.0, 2.0],
                      [float("-inf"), float("-inf"), float("-inf"), float("-inf")], [1.0, 2.0, 2.0, 0.0]])
    xs = x.T.reshape(1, 2, 2, 7).repeat(1, 1, 1, 4)[..., :28].contiguous()            # window position -> (row, column); C = 28
    out, which, dx = Sc.pool_reference(xs, torch.ones(1, 1, 1, 28))
    assert which[0, 0, 0, :7].tolist() == [0, 0, 0, 2, 1, 0, 1]
    assert torch.equal(out[0, 0, 0, 1].view(torch.int32), torch.tensor(0.0).view(torch.int32))        # +0 kept
    assert torch.equal(out[0, 0, 0, 2].view(torch.int32), torch.tensor(-0.0).view(torch.int32))       # the first, -0, kept
    assert float(dx.sum()) == 28.0 and Sc.pool_gap(xs[..., 6:7]) == 0.0
    for name, xc in Sc.pool_cases((2, 3, 5), 8, 1).items():
        o, w, _ = Sc.pool_reference(xc)
        win = xc.reshape(2, 3, 2, 5, 2, 8).permute(0, 1, 3, 5, 2, 4).reshape(2, 3, 5, 8, 4)
        picked = torch.gather(win, 4, w.long()[..., None])[..., 0]
        assert torch.equal(picked.view(torch.int32), o.view(torch.int32)), name


def test_fixture_against_the_restatements(fx):
    """The stored inputs regenerate, the recorded reference results lie within d_T of the restatement on the recorded rows, and
    the restatement of the whole stage agrees with float64 autograd over torch's own ops."""
    x2s, sp, dlogits = Sc.stage_inputs(fx)
    assert x2s.shape == (2, 16, 16, 64) and dlogits.shape == (2, 65, 8, 8)
    res = Sc.stage64(x2s, sp, dlogits)
    ag = Sc.stage_autograd64(x2s, sp, dlogits)
    for k in Sc.STAGE_GATED:
        assert Sc.err(ag[k], res[k], res["S"][k]) <= 1e-12, k
        d = float(fx[f"stage.d_{k}"])
        assert 0 < d < 1e-6 and Sc.tol(fx, "stage", k) == max(4 * d, Sc.TOL_FLOOR), k
        got, want = torch.from_numpy(fx[f"stage.model.{k}"]), Sc.recorded_part(res[k])
        assert Sc.err(got, want, res["S"][k]) <= d * (1 + 1e-9), k
    assert res["pool_gap"] == float(fx["stage.pool_gap"]) > Sc.POOL_FACTOR * float(fx["stage.pool_moved"])
    for name, h in res["kinks"].items():
        nz = h[h != 0].abs().min()
        assert float(nz) == float(fx[f"stage.kink.{name}"]) > float(fx[f"stage.moved.{name}"]), name
    for unit, cases, case, restate, gated in (("rcab", Sc.RCAB_CASES, Sc.rcab_case, R.restate64, R.GATED),
                                              ("gmlp", Sc.GMLP_CASES, Sc.gmlp_case, G.restate64, G.GATED)):
        worst = {k: 0.0 for k in gated}
        for name in cases:
            inputs = case(name)
            assert T.inputs_digest(*inputs) == str(fx[f"{unit}.{name}.inputs_sha256"]), (unit, name)
            res = restate(*inputs)
            for k in gated:
                got, want = torch.from_numpy(fx[f"{unit}.{name}.{k}"]), Sc.recorded_part(res[k])
                worst[k] = max(worst[k], Sc.err(got, want, res["S"][k]))
        for k in gated:
            assert worst[k] <= float(fx[f"{unit}.d_{k}"]) * (1 + 1e-9), (unit, k)
    # case edges holds its edges
    y, r, p, g = Sc.rcab_case("edges")
    res = R.restate64(y, r, p, g)
    assert bool((res["h"].reshape(3, 3, 5, C3)[R.EDGES_CONST_ROW][:R.EDGES_H0] == 0).all())
    assert float(res["se_pre"][:, R.EDGES_E0].abs().max()) == 0.0 and float(res["dws0"][R.EDGES_E0].abs().max()) == 0.0
