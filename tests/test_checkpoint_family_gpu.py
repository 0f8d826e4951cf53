"""The split-f16 forward on re-scaled checkpoints, small operands too.

Every other accuracy figure of the suite is taken on ONE weight distribution (synth.synthetic_state_dict); the guard tests push
operands UP only.  Here the family of tests/golden/cases.py goes through the module: exact power-of-two re-parameterisations of
every LayerNorm -> Linear pair of every stage (2^-k on the norm, 2^k on the Linear and the other way round, k up to 14, one pair
at a time and all pairs of a stage at once) and five changes of the weight distribution, on noise and on a crop of a photograph,
with the fall-back to the fp32 kernels allowed (BALF_FP16_STRICT lifted for this module): falling back is a legal outcome, a
score map more than 1e-4 off is not.

Expected values: the float64 oracle -- of the BASE member for the exact members (tests/test_checkpoint_family.py proves on the CPU
that the fp32 oracle is bit-identical for every one of them on this very input), of the member itself for the others.

What was found (profiles/checkpoint_family.json, DESIGN.md "operand range"): the channel pairs (rsh, grid, block, rcab) are folded
into one matrix when the weights are packed, so their re-parameterisations never reach a kernel.  The gating unit's norm -> token
mix is not folded, and before the packer normalised it by a power of two (weights.hip: gate_pair_scale) the split path was 6.7e-5
off at k = 12, stayed on fp16 with 1.34e-4 at grid_gate.s1.up10 (probes passed: the hole), and was sent to fp32 by the probes only
from k = 12 / 14 on.  With the normalisation every exact member packs to the base member's operands and the split path returns the
base member's bits, which test_member asserts.

One member stays on the split path beyond ``tol`` and is asserted against 1e-4 only, see NAMED."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.golden import cases
from tests.test_forward_gpu import TIGHT_PROB          # the fp32 gate of test_forward_gpu.py (5e-6, against the fp32 reference)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("checkpoint_family", os.path.join(ROOT, "tools", "checkpoint_family.py"))
cf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cf)

MEMBERS = cases.family_exact_members() + cases.family_dist_members()
STAGE_GATE = 2e-5        # relative, tests/test_stage_parity_gpu.py: GATE
# Members that stay on the split path with an error between tol = max(2e-5, 4 e32) and the 1e-4 contract: asserted against 1e-4.
#   row_gains_rms: 2.63e-5 on the split path with e32 = 4.97e-6 (tol 2.0e-5).  Not the split: the exact-fp32 KERNELS are 2.18e-5
#   off on it too (rows of one matrix differ by up to 2^8, which amplifies what both kernel families share, the GELU table).
NAMED = {"row_gains_rms"}


@pytest.fixture(scope="module")
def fam():
    return cf.Family()


@pytest.fixture(autouse=True)
def _fallback_allowed(monkeypatch):
    monkeypatch.delenv("BALF_FP16_STRICT", raising=False)        # (conftest sets it; falling back is a legal outcome here)
    monkeypatch.setenv("BALF_FP16_GUARD", "sync")                # a flagged batch is repaired before forward returns


@pytest.fixture(scope="module")
def base_out(fam):
    """The base member's score map from each kernel family."""
    out = {p: fam.run(cases.FAMILY_BASE, p) for p in ("fp16", "fp32")}
    assert out["fp16"][0]["effective"] == "fp16" and out["fp32"][0]["effective"] == "fp32"
    return {p: v[1] for p, v in out.items()}


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("member", MEMBERS, ids=[m[0] for m in MEMBERS])
def test_member(fam, base_out, member, precision):
    row, prob = fam.run(member, precision)
    print(row)
    exact = member[1] == "exact"
    # the contract, whatever the module ended on
    assert row["finite"] and row["err"] <= cf.CONTRACT, row
    if precision == "fp32":
        assert row["effective"] == "fp32"
        if exact:
            assert row["err"] <= max(TIGHT_PROB, 2.0 * row["e32"]), row
            # the exact-fp32 kernels are scale-exact: the gate pairs reach them un-normalised (the packer rescales the split-f16
            # blob only) and the channel pairs folded, and either way the bits are the base member's
            assert np.array_equal(prob, base_out["fp32"]), row
        return
    # the status block of the split kernels on these weights, read independently of the module's own guard: what tripped it or
    # produced a non-finite value must have ended on the fp32 kernels
    if any(row["status"]) or not row["split_finite"]:
        assert row["effective"] == "fp32", row
    if exact:
        # stronger than the contract asks, and what makes the bit-identity below non-vacuous: the packer hands the split kernels
        # the base member's operands, so there is nothing for the probes to object to
        assert row["effective"] == "fp16", row
    if row["effective"] == "fp16":
        assert not row["warned"], row
        assert row["err"] <= (cf.CONTRACT if member[0] in NAMED else row["tol"]), row
        if exact:
            # a power-of-two re-parameterisation is harmless BY CONSTRUCTION: folded (channel pairs) or normalised (gate pairs)
            # when the weights are packed, so the kernels see the base member's operands
            assert np.array_equal(prob, base_out["fp16"]), row
    else:
        assert row["effective"] == "fp32" and row["warned"], row


def _stage_refs(fam):
    """The base member's stage outputs from the float64 oracle, NHWC: down1..down3 and x2 of down4 (what stage_view returns)."""
    sd = O.cast_state(fam.sd0, torch.float64)
    t = fam.x.double().permute(0, 2, 3, 1)
    refs, taps = [], {}
    with torch.no_grad():
        for s in range(4):
            t = O.stage_forward(sd, f"down{s + 1}", t, last=(s == 3), taps=taps)
            refs.append((t if s < 3 else taps["down4.x2"]).numpy())
    return refs


@pytest.fixture(scope="module")
def stage_refs(fam):
    return _stage_refs(fam)


KMAX = max(cases.FAMILY_KS)
FARTHEST = [m for m in cases.family_exact_members() if m[2][1] == KMAX]


@pytest.mark.parametrize("member", FARTHEST, ids=[m[0] for m in FARTHEST])
def test_stage_outputs_of_the_farthest_members(fam, stage_refs, member):
    """Localisation: every pair of every stage at the largest k, both directions (before the packer's normalisation the error
    grew with k, so these were the worst member of each pair): the activations at the stage boundaries against the float64
    oracle's, so that a failure names the stage.  Gate of tests/test_stage_parity_gpu.py."""
    row, _ = fam.run(member, "fp16")
    b, _, h, w = fam.x.shape
    m = fam.model("fp16")
    views = [v.cpu().numpy() for v in m.stage_view(b, h, w)]       # (of the module's own forward inside run)
    for s in range(4):
        ref = stage_refs[s]
        assert views[s].shape == ref.shape
        rel = float(np.abs(views[s] - ref).max() / max(1.0, np.abs(ref).max()))
        print(f"{member[0]} ({row['effective']}) down{s + 1}: rel {rel:.2e}")
        assert rel < STAGE_GATE, (member[0], row["effective"], f"down{s + 1}", rel)


@pytest.mark.parametrize("name", ["all.s1.up14", "grid_gate.s1.up10", "row_gains_rms"])
def test_worst_members_are_deterministic(fam, name):
    """all.s1.up14: the largest error of the split kernels before the normalisation (2.1e-3); grid_gate.s1.up10: the member that
    broke the contract; row_gains_rms: the largest error of a member kept on the split path now."""
    member = next(m for m in MEMBERS if m[0] == name)
    (r1, p1), (r2, p2) = fam.run(member, "fp16"), fam.run(member, "fp16")
    assert r1["effective"] == r2["effective"] and np.array_equal(p1, p2)
