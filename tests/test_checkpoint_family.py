"""The checkpoint family of tests/golden/cases.py, pinned on the CPU (no GPU needed).

The exact members re-parameterise a LayerNorm -> Linear pair by a power of two; the GPU tests (test_checkpoint_family_gpu.py) take
the BASE member's float64 output as the expected value of every one of them.  That is right only if the reference itself computes
the same function: here the fp32 oracle's ``prob`` and ``logits`` must be bit-identical to the base member's, member by member, on
the GPU tests' own input (noise + photograph, 128x192) and on a 64x64 batch.  A member that failed would be dropped from the family
in cases.py; none does, and the grid test below pins that every (pair, stage, direction, k) is still there."""
import os

import pytest
import torch

from balf_amd.utils import synth
from oracle import oracle as O
from tests.golden import cases

G = os.path.join(os.path.dirname(__file__), "golden")
EXACT = cases.family_exact_members()


@pytest.fixture(scope="module")
def base():
    sd = synth.synthetic_state_dict(cases.WEIGHT_SEED)
    xs = [cases.family_input(G), cases.forward_input(2, 64, 64, 41)]
    with torch.no_grad():
        return sd, xs, [O.detector_forward(sd, x) for x in xs]


def test_family_grid_is_complete():
    """Every pair (and "all pairs of the stage") in every stage, both directions, every k of the sweep 0, 4, 8, 10, 12, 14; distinct ids."""
    ids = [m[0] for m in EXACT + cases.family_dist_members()]
    assert len(set(ids)) == len(ids)
    assert set(cases.FAMILY_KS) >= {0, 4, 8, 10, 12, 14} and cases.FAMILY_STAGES == (1, 2, 3, 4)
    assert set(cases.FAMILY_PAIRS) == {"rsh", "grid", "block", "rcab", "grid_gate", "block_gate"}
    want = {f"{p}.s{s}.{d}{k}" for p in list(cases.FAMILY_PAIRS) + ["all"] for s in cases.FAMILY_STAGES
            for d in cases.FAMILY_DIRECTIONS for k in cases.FAMILY_KS if k} | {"base"}
    assert set(m[0] for m in EXACT) == want and len(want) == 1 + 7 * 4 * 2 * 5
    assert cases.FAMILY_BASE in EXACT and cases.FAMILY_BASE[2][1] == 0


def test_members_touch_what_they_name(base):
    sd = base[0]
    for m in EXACT:
        msd = cases.family_state(sd, m)
        changed = sorted(k for k in sd if not torch.equal(msd[k], sd[k]))
        assert changed == sorted(cases.family_touched_keys(m)), m[0]
        d, k, pairs = m[2]
        for n, l in pairs:                     # powers of two, and the product of the two scales is exactly one
            assert torch.equal(msd[n + ".weight"] * msd[l + ".weight"][:1, :1], sd[n + ".weight"] * sd[l + ".weight"][:1, :1])
            assert torch.equal(msd[l + ".bias"], sd[l + ".bias"])
    for m in cases.family_dist_members():
        msd = cases.family_state(sd, m)
        assert set(msd) == set(sd) and any(not torch.equal(msd[k], sd[k]) for k in sd), m[0]
        assert all(msd[k].dtype == sd[k].dtype and msd[k].shape == sd[k].shape for k in sd)
        assert all(bool(torch.isfinite(v).all()) for v in msd.values() if v.is_floating_point())


@pytest.mark.parametrize("member", EXACT[1:], ids=[m[0] for m in EXACT[1:]])
def test_exact_member_is_bit_identical_in_the_fp32_reference(base, member):
    sd, xs, want = base
    msd = cases.family_state(sd, member)
    with torch.no_grad():
        for x, w in zip(xs, want):
            got = O.detector_forward(msd, x)
            assert torch.equal(got["prob"], w["prob"]) and torch.equal(got["logits"], w["logits"]), member[0]


def test_distribution_members_change_the_function(base):
    """... and stay finite in the fp32 reference (a member the reference cannot compute would test nothing)."""
    sd, xs, want = base
    for m in cases.family_dist_members():
        with torch.no_grad():
            got = O.detector_forward(cases.family_state(sd, m), xs[0])
        assert bool(torch.isfinite(got["logits"]).all()) and not torch.equal(got["prob"], want[0]["prob"]), m[0]


def test_gate_pairs_pack_to_the_base_members_split_operands(base):
    """The gating unit's norm -> token mix is the one pair the packer does not fold into one matrix; it normalises the pair by a
    power of two instead (weights.hip: gate_pair_scale), so a re-parameterised checkpoint reaches the split-f16 kernels with the
    base member's operands: the packed blob is byte-identical.  The synthetic checkpoint itself is left alone (scale 1), and the
    fp32 blob is never rescaled (those kernels are scale-exact, test_checkpoint_family_gpu.py)."""
    from balf_amd import arch
    from balf_amd.model import get_model
    sd = base[0]
    m = get_model.load_model(arch.DEFAULT_MODEL_CFG).eval()

    def blob(msd, precision):
        m.load_state_dict(msd)
        return m.packed_weights("cpu", precision).clone()
    b16, b32 = blob(sd, "fp16"), blob(sd, "fp32")
    for member in EXACT[1:]:
        if member[0].split(".")[0] not in ("grid_gate", "block_gate"):
            continue
        msd = cases.family_state(sd, member)
        assert torch.equal(blob(msd, "fp16"), b16), member[0]
        assert not torch.equal(blob(msd, "fp32"), b32), member[0]
    # inside the band [1/4, 4) nothing is rescaled: x2 on the norm reaches the kernels as x2
    for pair in ("grid_gate", "block_gate"):
        n, l = (f"down2.{v}" for v in cases.FAMILY_PAIRS[pair])
        msd = dict(sd)
        msd[n + ".weight"], msd[n + ".bias"], msd[l + ".weight"] = sd[n + ".weight"] * 2, sd[n + ".bias"] * 2, sd[l + ".weight"] / 2
        assert not torch.equal(blob(msd, "fp16"), b16)
