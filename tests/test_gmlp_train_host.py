"""The parts of the gMLP training path that need no GPU: the fixture gmlp_train.npz and its gates, the float64 restatement
against float64 autograd over the oracle's arithmetic, what the ``layout`` and ``edges`` cases must show, the argument checks of
the C ABI and of the Python wrappers, ``GMLP_PARAMS`` against the model, and TrainableMixerTail's state handling."""
import ctypes as C
import os

import pytest
import torch

from balf_amd import _lib, arch, ops
from balf_amd.model import get_model
from balf_amd.model.mixer_train import TrainableMixerTail
from balf_amd.utils import synth
from tests import gmlp_train_common as G


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fx():
    return G.fixture()


@pytest.fixture(scope="module")
def cases(fx):
    """name -> (inputs, restate64 of them), computed once."""
    out = {}
    for name in G.FIXTURE_CASES:
        c = G.fixture_case(fx, name)
        out[name] = (c, G.restate64(*c))
    return out


def test_fixture_digest_and_gates(fx):
    assert list(fx["meta.names"]) == list(G.FIXTURE_CASES)
    assert os.path.getsize(G.FIXTURE) < 1000000
    for name in G.FIXTURE_CASES:
        assert str(fx[f"{name}.inputs_sha256"]) == G.regenerated_inputs_digest(name), name
    for k in G.GATED:
        d, tol = float(fx[f"d_{k}"]), float(fx[f"tol_{k}"])
        assert tol == max(4 * d, G.TOL_FLOOR) and 0 < d < 1e-6, (k, d, tol)
    assert fx["model.x0"].shape == (2, 8, 8, 256) and bool((fx["model.x0"] >= 0).all())


def test_params_match_the_model():
    assert tuple(G.PARAMS) == tuple(ops.GMLP_PARAMS) and len(ops.GMLP_PARAMS) == 26
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    sd = model.state_dict()
    own = [k[len(G.SD_PREFIX):] for k in sd if k.startswith(G.SD_PREFIX)]
    assert own == list(ops.GMLP_PARAMS)                         # the names, and the state dict's own order
    for k in ops.GMLP_PARAMS:
        assert tuple(sd[G.SD_PREFIX + k].shape) == ops._GMLP_PARAM_SHAPES[k], k
    assert sum(sd[G.SD_PREFIX + k].numel() for k in ops.GMLP_PARAMS) == 668544


@pytest.mark.parametrize("name", G.FIXTURE_CASES)
def test_restatement_against_autograd_and_the_recorded_reference(fx, cases, name):
    (x0, p, g), res = cases[name]
    ag = G.autograd64(x0, p, g)
    for k in G.GRADS:
        assert G.err(ag[k], res[k], res["S"][k]) <= 1e-12, k
    y64 = G._compose(x0.double(), {k: v.double() for k, v in p.items()})
    assert G.err(y64, res["y"], res["S"]["y"]) <= 1e-12
    for k in G.GATED:                                           # the reference's own float32 results, as recorded
        if name == "model" and k == "dx0":
            continue                                            # recorded as dx0_full, with the long shortcut's share
        ref, mine = G.recorded(fx, name, k, res[k])
        e = G.err(ref, mine, res["S"][k])
        assert e <= float(fx[f"d_{k}"]) * (1 + 1e-6) + 1e-15 <= float(fx[f"tol_{k}"]), (k, e)
    # the float32 torch-op composition (what tools/bench_gmlp_train.py times) states the same function
    y, g32 = G.compose_f32(x0, p, g)
    assert G.err(y, res["y"], res["S"]["y"]) <= float(fx["tol_y"])
    for k in G.GRADS:
        assert G.err(g32[k], res[k], res["S"][k]) <= float(fx[f"tol_{k}"]), k


def test_token_maps():
    """Both maps are permutations of the pixels, a group never spans two images, and at Hc = Wc = 8 they are the same map."""
    for b, hc, wc in ((1, 8, 8), (2, 16, 24), (3, 8, 16)):
        for grid in (True, False):
            idx = G.token_index(b, hc, wc, grid)
            assert idx.shape == (b * hc * wc // 64, 64) and sorted(idx.reshape(-1).tolist()) == list(range(b * hc * wc))
            img = idx // (hc * wc)
            assert bool((img == img[:, :1]).all())
    assert torch.equal(G.token_index(2, 8, 8, True), G.token_index(2, 8, 8, False))
    assert not torch.equal(G.token_index(1, 16, 24, True), G.token_index(1, 16, 24, False))
    # token 9 of the first group: region (1, 1) of 2 x 3 pixels under the grid map, pixel (1, 1) of the block under the block map
    assert int(G.token_index(1, 16, 24, True)[0, 9]) == 2 * 24 + 3 and int(G.token_index(1, 16, 24, False)[0, 9]) == 24 + 1


def test_layout_case_tells_the_maps_and_the_orientation_apart(fx, cases):
    """A wrong map, the two maps exchanged, or Wt transposed each move y of case ``layout`` far outside its gate."""
    (x0, p, g), res = cases["layout"]
    tol = float(fx["tol_y"])
    gl, gu = G.BRANCHES[0]
    bl, bu = G.BRANCHES[1]
    for k in (f"{gl}.{gu}.dense.weight", f"{bl}.{bu}.dense.weight"):
        q = dict(p)
        q[k] = p[k].T.contiguous()
        assert G.err(G.restate64(x0, q)["y"], res["y"], res["S"]["y"]) > 1e4 * tol, k
    swapped = dict(p)                                           # the branches exchanged = each half mixed under the other map
    for n in G._BRANCH:
        a, b = f"{gl}.{n.format(u=gu)}", f"{bl}.{n.format(u=bu)}"
        swapped[a], swapped[b] = p[b], p[a]
    assert G.err(G.restate64(x0, swapped)["y"], res["y"], res["S"]["y"]) > 1e4 * tol


def test_restatement_edges(cases):
    """What the ``edges`` case must show."""
    (x0, p, g), res = cases["edges"]
    gl, gu = G.BRANCHES[0]
    bl, bu = G.BRANCHES[1]
    row = x0[G.EDGES_CONST_ROW].double()
    assert bool((row == row[0]).all())                          # var = 0, xhat = 0 exactly
    assert res["S"][f"d:{gl}.{gu}.norm.weight"] == 0.0 and bool((res[f"d:{gl}.{gu}.norm.weight"] == 0).all())
    assert float(res[f"d:{gl}.{gu}.norm.bias"].abs().max()) > 0
    # the block map's token with a zero row of Wt and bt = -1: mix + 1 == 0, so its dWt row and dbt still move, its gate is shut
    assert bool((p[f"{bl}.{bu}.dense.weight"][G.EDGES_GATE0] == 0).all()) and float(p[f"{bl}.{bu}.dense.bias"][G.EDGES_GATE0]) == -1.0
    assert float(res[f"d:{bl}.{bu}.dense.bias"][G.EDGES_GATE0].abs()) > 0
    for k in (f"{gl}.norm.weight", f"{gl}.{gu}.norm.weight", "norm.weight"):
        assert float(p[k][G.EDGES_GAIN0]) == 0.0
    for k in (f"d:{gl}.norm.weight", "d:norm.weight"):          # the gradient of a zero gain is no zero
        assert float(res[k][G.EDGES_GAIN0].abs()) > 1e-3 * res["S"][k], k
    h0, hb = res["h0"], res["hb"][1]
    for c, v in G.EDGES_SAT[256]:                                    # saturated both ways, inside the normal range
        for h in (h0, hb):
            assert bool((h[:, c] > 3).all()) if v > 0 else bool((h[:, c] < -3).all())
            assert float(h[:, c].abs().max()) > 9 and float(h.abs().max()) < 40
        assert 0 < float(G._gelu_grad(h0[:, c]).sub(1.0 if v > 0 else 0.0).abs().max()) < 0.02


def test_abi_argument_checks(lib):
    fake = C.c_void_p(4096)
    shape = (2, 8, 16)
    n = 2 * 8 * 16
    ws, sv = lib.balf_gmlp_train_workspace_bytes(*shape), lib.balf_gmlp_train_saved_bytes(*shape)
    assert ws > 0 and sv >= n * (256 + 3 * 512 + 2 * (4 * 256 + 2 * 512)) * 4
    ptrs = lambda hole=None: (C.c_void_p * 26)(*[None if i == hole else 4096 for i in range(26)])      # noqa: E731

    def fwd(dims=shape, nbytes=ws, x=fake, params=None, y=fake, saved=fake, work=fake):
        return lib.balf_gmlp_train_forward(x, params if params is not None else ptrs(), *dims, y, saved, work, nbytes, None)

    def bwd(dims=shape, nbytes=ws, dy=fake, x=fake, params=None, saved=fake, grads=None, dx0=None, work=fake):
        return lib.balf_gmlp_train_backward(dy, x, params if params is not None else ptrs(), saved, *dims,
                                            grads if grads is not None else ptrs(), dx0, work, nbytes, None)

    null = C.POINTER(C.c_void_p)()
    for k in ("x", "y", "saved", "work"):
        assert fwd(**{k: None}) == -1, k
    for k in ("dy", "x", "saved", "work"):
        assert bwd(**{k: None}) == -1, k
    assert fwd(params=null) == -1 and bwd(params=null) == -1 and bwd(grads=null) == -1
    for hole in (0, 11, 25):
        assert fwd(params=ptrs(hole)) == -1 and bwd(params=ptrs(hole)) == -1 and bwd(grads=ptrs(hole)) == -1
    odd = (C.c_void_p * 26)(*[4100 if i == 4 else 4096 for i in range(26)])
    assert fwd(params=odd) == -1 and bwd(params=odd) == -1
    for call in (fwd, bwd):
        assert call(dims=(0, 8, 8)) == -1 and call(dims=(65536, 8, 8)) == -1 and call(dims=(1, 0, 8)) == -1 and call(dims=(1, 8, -8)) == -1
        assert call(dims=(1, 12, 8)) == -2 and call(dims=(1, 8, 12)) == -2 and call(dims=(1, 4, 4)) == -2
        assert call(dims=(4097, 64, 64), nbytes=1 << 60) == -2      # N > 2^24
        assert call(work=C.c_void_p(4104)) == -1 and call(saved=C.c_void_p(4104)) == -1 and call(x=C.c_void_p(4100)) == -1
        assert call(nbytes=ws - 1) == -3
    assert fwd(y=C.c_void_p(4100)) == -1 and bwd(dy=C.c_void_p(4100)) == -1 and bwd(dx0=C.c_void_p(4100)) == -1
    for query in (lib.balf_gmlp_train_workspace_bytes, lib.balf_gmlp_train_saved_bytes):
        assert [query(*bad) for bad in ((0, 8, 8), (1, 12, 8), (1, 8, 4), (4097, 64, 64), (65536, 8, 8), (2, 0, 8))] == [0] * 6
        sizes = [query(1, 8, v) for v in (8, 16, 64, 256, 2048, 1 << 14, 1 << 21)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # balf_forward_gmlp_input: the residency rules and codes of balf_forward_stage_view
    fb = lib.balf_forward_workspace_bytes(2, 64, 64)

    def inp(prec=1, nbytes=fb, b=2, hp=64, wp=64, **kw):
        a = dict(ws=fake, w=fake, bias=fake, x0=fake, scratch=fake)
        a.update(kw)
        return lib.balf_forward_gmlp_input(prec, a["ws"], nbytes, b, hp, wp, a["w"], a["bias"], a["x0"], a["scratch"], None)

    for k in ("ws", "w", "bias", "x0", "scratch"):
        assert inp(**{k: None}) == -1, k
    assert inp(prec=7) == -1 and inp(b=0) == -1
    assert inp(hp=60) == -2
    assert inp(nbytes=fb - 1) == -3
    assert inp(b=17, hp=1088, wp=1920, nbytes=1 << 40) == -1       # 17 images: two micro-batches, the first is gone


def test_python_layers_refuse_before_touching_a_device():
    x0, p, dy = G.sweep_case((1, 8, 8), 1)
    params = [p[k] for k in G.PARAMS]
    saved = torch.zeros(1 << 20, dtype=torch.uint8)
    with pytest.raises(_lib.BalfHipError, match="GPU"):                      # CPU tensors
        ops.gmlp_train_forward(x0, params)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.gmlp_train_backward(dy, x0, params, saved)
    with pytest.raises(_lib.BalfHipError, match="26 parameters"):
        ops.gmlp_train_forward(x0, params[:25])
    for i, k in enumerate(G.PARAMS):
        with pytest.raises(_lib.BalfHipError, match=f"{k} must be float32"):
            ops.gmlp_train_forward(x0, params[:i] + [params[i].double()] + params[i + 1:])
        with pytest.raises(_lib.BalfHipError, match=f"{k} must be"):
            ops.gmlp_train_forward(x0, params[:i] + [params[i][:32].contiguous()] + params[i + 1:])
    with pytest.raises(_lib.BalfHipError, match="float32"):
        ops.gmlp_train_forward(x0.double(), params)
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.gmlp_train_forward(x0.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), params)
    with pytest.raises(_lib.BalfHipError, match="contiguous"):
        ops.gmlp_train_forward(x0, params[:12] + [params[12].T] + params[13:])
    with pytest.raises(_lib.BalfHipError, match="256"):
        ops.gmlp_train_forward(x0[..., :128].contiguous(), params)
    for bad in ((1, 12, 8, 256), (1, 8, 4, 256), (0, 8, 8, 256)):
        with pytest.raises(_lib.BalfHipError, match="multiples of 8"):
            ops.gmlp_train_forward(torch.zeros(bad), params)
    with pytest.raises(_lib.BalfHipError, match="16-byte"):                  # a view one float into its storage
        ops.gmlp_train_forward(torch.zeros(x0.numel() + 1)[1:].view(x0.shape), params)
    with pytest.raises(_lib.BalfHipError, match="dy must be"):
        ops.gmlp_train_backward(dy[..., :128].contiguous(), x0, params, saved)
    with pytest.raises(_lib.BalfHipError, match="float32"):
        ops.gmlp_train_backward(dy.half(), x0, params, saved)
    with pytest.raises(_lib.BalfHipError, match="dx0 must be"):
        ops.gmlp_train_backward(dy, x0, params, saved, want_dx0=torch.zeros(1, 8, 8, 128))
    with pytest.raises(_lib.BalfHipError, match="saved"):
        ops.gmlp_train_backward(dy, x0, params, saved.float())
    ws = torch.zeros(16, dtype=torch.uint8)
    w0, b0 = torch.zeros(256, 128), torch.zeros(256)
    out = torch.zeros(1, 8, 8, 256)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        ops.gmlp_input(_lib.PREC_FP32, ws, 1, 64, 64, w0, b0, out)
    with pytest.raises(_lib.BalfHipError, match="conv0_w must be"):
        ops.gmlp_input(_lib.PREC_FP32, ws, 1, 64, 64, w0.T.contiguous(), b0, out)
    with pytest.raises(_lib.BalfHipError, match="x0 must be"):
        ops.gmlp_input(_lib.PREC_FP32, ws, 1, 64, 64, w0, b0, out[..., :128].contiguous())
    with pytest.raises(_lib.BalfHipError, match="multiples of 64"):
        ops.gmlp_input(_lib.PREC_FP32, ws, 1, 60, 64, w0, b0, out)
    mixer = TrainableMixerTail()
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        mixer(x0)
    with pytest.raises(_lib.BalfHipError, match="GPU"):
        mixer.eval()(x0)
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    with pytest.raises(_lib.BalfHipError, match="CPU"):
        model.encode(torch.zeros(1, 3, 64, 64), level="gmlp")


def test_trainable_mixer_tail_state():
    model = get_model.load_model(arch.DEFAULT_MODEL_CFG)
    sd = synth.synthetic_state_dict(2)
    model.load_state_dict(sd)
    mixer = TrainableMixerTail.from_model(model)
    assert mixer.training and mixer.tail.training and mixer.tail.head.training and mixer.encode_level == "gmlp"
    state = mixer.state_dict()
    assert list(state)[:26] == ["mixer." + k for k in ops.GMLP_PARAMS]
    assert list(state)[26:] == ["tail." + k for k in mixer.tail.state_dict()]
    assert len(list(mixer.parameters())) == 26 + 16 and sum(q.numel() for q in mixer.gmlp_parameters()) == 668544
    for k in ops.GMLP_PARAMS:
        mine = state["mixer." + k]
        assert torch.equal(mine, sd[G.SD_PREFIX + k]) and mine.data_ptr() != model.state_dict()[G.SD_PREFIX + k].data_ptr(), k
    key = model._weights_key("cpu")
    with torch.no_grad():                                                # what an optimiser step does to the copies
        for q in mixer.parameters():
            q.add_(1.0)
    assert model._weights_key("cpu") == key
    assert torch.equal(model.state_dict()[G.SD_PREFIX + "dense1.weight"], sd[G.SD_PREFIX + "dense1.weight"])
    mixer.commit(model)
    assert model._weights_key("cpu") != key
    after = model.state_dict()
    for k in ops.GMLP_PARAMS:
        assert torch.equal(after[G.SD_PREFIX + k], sd[G.SD_PREFIX + k] + 1.0), k
    rcab = "down4.residual_channel_attention_block.conv1.weight"
    assert torch.equal(after[rcab], sd[rcab] + 1.0) and torch.equal(after["down4.conv2.weight"], sd["down4.conv2.weight"] + 1.0)
    assert torch.equal(after["down4.conv.0.weight"], sd["down4.conv.0.weight"])               # down4.conv.0 stays frozen
    other = "down3.residual_split_head_multi_axis_gmlp_layer.dense2.weight"
    assert torch.equal(after[other], sd[other])
    mixer.eval()
    assert not mixer.tail.training and not mixer.tail.head.training
