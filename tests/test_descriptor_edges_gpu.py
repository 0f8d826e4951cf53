"""The descriptor leg at its hard edges: csrc/match.hip, csrc/patches.hip and the masked-slot path of
csrc/hardnet.hip against plain float64 references (tests/descriptor_common.py, themselves tested on the CPU in
tests/test_descriptor_edges_host.py), and their caller-owned buffers through the C ABI with guard bands at exactly the
documented sizes and over poisoned workspaces.  These pin the arithmetic to the documented algorithm, not to kornia."""
import functools

import numpy as np
import pytest
import torch

from balf_amd import _lib, ops
from balf_amd.third_party.hardnet.hardnet_pytorch import HardNet
from balf_amd.utils import synth
from oracle import oracle
from tests import descriptor_common as DC
from tests.golden import cases
from tests.test_guard_gpu import Guarded, _stream
from tests.test_hardnet_gpu import DESC_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_WORKSPACE = -3


def _gpu_match(d1, d2, th):
    gd, gi = ops.match_smnn(torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV), th)
    assert gi.dtype == torch.int64 and gd.shape == (gi.shape[0], 1)
    return gi.cpu().numpy(), gd.cpu().numpy().reshape(-1)


# ---- matcher --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,scale", DC.NEAR_CASES)
def test_match_near_duplicates_within_the_fp32_contract(sigma, scale):
    """d^2 = |a|^2 + |b|^2 - 2 a.b cancels to ~128 sigma^2 here.  On rows the contract decides the match set is the fp64
    reference's, every dist is within the ratio error the contract implies, and nothing is reported that the reference
    decidedly excludes.  An operand type narrower than fp32 in the MFMA (error ~2^-11 |a||b|) fails this at sigma 1e-3."""
    d1, d2, src, _ = DC.near_duplicate_case(sigma, scale)
    ref = DC.MatchRef(d1, d2, DC.NEAR_TH)
    gi, gd = _gpu_match(d1, d2, DC.NEAR_TH)
    n_decided, _ = ref.check(gi, gd)
    assert n_decided >= 0.9 * DC.NEAR_SOURCES and set(gi[:, 0].tolist()) <= set(src.tolist())


@pytest.mark.parametrize("n1,n2", DC.SWEEP_SHAPES)
def test_match_shapes_around_the_tiles(n1, n2):
    d1, d2, perm = DC.sweep_case(n1, n2)
    ref = DC.MatchRef(d1, d2, DC.SWEEP_TH)
    gi, gd = _gpu_match(d1, d2, DC.SWEEP_TH)
    ref.check(gi, gd)
    if min(n1, n2) < 2:
        assert len(gi) == 0
    if perm is not None:                # every row matches: count == cap, past the 1024-row step of the mutual kernel
        assert len(gi) == n1 == min(n1, n2)
        assert np.array_equal(gi[:, 0], np.arange(n1)) and np.array_equal(gi[:, 1], np.argsort(perm))


def test_match_ties_go_to_the_lowest_index():
    """th = 1.0 and exact duplicates at a non-zero distance: the tied row's ratio is exactly 1 and passes, so the index
    best_insert / best_merge picked is in the output.  Identical columns get identical distances, whichever lane or tile
    they are in, so the whole index list equals the reference's (the other rows are decided by wide gaps)."""
    d1, d2 = DC.tie_case()
    for a, b, swapped in ((d1, d2, False), (d2, d1, True)):
        ref = DC.MatchRef(a, b, 1.0)
        gi, gd = _gpu_match(a, b, 1.0)
        got = {tuple(r) for r in gi.tolist()}
        for i, (ja, jb) in enumerate(DC.TIE_PAIRS):
            lo, hi = ((ja, i), (jb, i)) if swapped else ((i, ja), (i, jb))
            assert lo in got and hi not in got, f"tie between columns {ja} and {jb} (roles swapped: {swapped})"
        assert np.array_equal(gi, ref.idx)
        assert np.abs(gd - ref.dist).max() < 1e-5


def _bad_rows(d, free):
    bad = d.copy()
    bad[free[0]] = np.nan
    bad[free[1], 7] = np.inf
    bad[free[2]] = 0.0
    return bad


@pytest.mark.parametrize("side", ["desc2", "desc1"])
def test_match_ignores_non_finite_rows(side):
    """One all-NaN row, one row with a +Inf and one all-zero row: as in the oracle (NaN sorts last in topk) a NaN distance
    is nobody's nearest or second-nearest neighbour, and the matches among the other rows are the ones of the run without
    the bad rows.  (fmaxf(d2, 0) used to turn the NaN into the best distance there is: the NaN row took every match.)"""
    d1, d2, src, dst = DC.near_duplicate_case(1e-2, 1.0)
    clean_i, clean_d = _gpu_match(d1, d2, DC.NEAR_TH)
    if side == "desc2":
        free = np.setdiff1d(np.arange(DC.NEAR_N2), dst)[:3]
        b1, b2, col = d1, _bad_rows(d2, free), 1
    else:
        free = np.setdiff1d(np.arange(DC.NEAR_N1), src)[:3]
        b1, b2, col = _bad_rows(d1, free), d2, 0
    assert not np.isin(clean_i[:, col], free).any() and len(clean_i) >= 0.9 * DC.NEAR_SOURCES
    gi, gd = _gpu_match(b1, b2, DC.NEAR_TH)
    ref = DC.MatchRef(b1, b2, DC.NEAR_TH)
    n_decided, _ = ref.check(gi, gd)
    assert n_decided >= 0.9 * DC.NEAR_SOURCES
    keep = ~np.isin(gi[:, col], free)
    assert not np.isin(gi[:, col], free[:2]).any()                 # the NaN and the Inf row match nothing
    assert np.array_equal(gi[keep], clean_i)                       # every (i, j) pair's distance is computed on its own
    assert np.isfinite(gd).all()


def _batch_descs(p, k, n1, n2, seed):
    rng = np.random.default_rng(seed)
    d1 = np.stack([DC.unit_rows(k, seed + 10 + i) for i in range(p)])
    d2 = np.stack([DC.unit_rows(k, seed + 50 + i) for i in range(p)])
    for i in range(p):                                    # plant correspondences inside the valid ranges
        m = min(n1[i], n2[i]) // 2
        if m:
            noisy = d1[i, :m] + 0.1 * rng.standard_normal((m, 128)).astype(np.float32)
            d2[i, n2[i] - m:n2[i]] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    return d1, d2


def test_match_batch_accepts_strided_views():
    """full[:, :k] of a wider K and full[::2]: the library strides pairs by K * 128 floats, so the wrapper has to hand it
    contiguous memory.  (The wrapper used to refuse such a view outright -- its own .float() made no copy of an fp32
    view, so handing it on would have matched every pair but the first on the wrong rows.)  ops.match_smnn likewise."""
    k, wide = 70, 96
    n1, n2 = np.array([70, 33, 64, 17], np.int32), np.array([70, 70, 40, 70], np.int32)
    w1, w2 = _batch_descs(4, wide, n1, n2, 3)
    f1, f2 = torch.from_numpy(w1).to(DEV), torch.from_numpy(w2).to(DEV)
    e1, e2 = torch.from_numpy(np.repeat(w1, 2, axis=0)).to(DEV), torch.from_numpy(np.repeat(w2, 2, axis=0)).to(DEV)
    e1[1::2] = 0.5
    e2[1::2] = -0.5
    t1, t2 = torch.from_numpy(n1), torch.from_numpy(n2)
    for v1, v2 in ((f1[:, :k], f2[:, :k]), (e1[::2], e2[::2]), (e1[::2, :k], e2[::2, 3:3 + k])):
        assert not v1.is_contiguous() and not v2.is_contiguous()
        m2 = torch.minimum(t2, torch.tensor(v2.shape[1], dtype=torch.int32))
        dist, idx, count = ops.match_smnn_batch(v1, t1, v2, m2, 0.95)
        rdist, ridx, rcount = ops.match_smnn_batch(v1.contiguous(), t1, v2.contiguous(), m2, 0.95)
        assert int(rcount.min()) > 0
        assert torch.equal(count, rcount) and torch.equal(idx, ridx) and torch.equal(dist, rdist)
        for p in range(4):                                # and the contiguous result is the per-pair reference's
            c = int(count[p])
            ref = DC.MatchRef(v1[p, :n1[p]].cpu().numpy(), v2[p, :int(m2[p])].cpu().numpy(), 0.95)
            ref.check(idx[p, :c].cpu().numpy(), dist[p, :c].cpu().numpy(), note=lambda s: None)
            sd, si = ops.match_smnn(v1[p, :n1[p]], v2[p][:int(m2[p])], 0.95)          # row views of one pair
            assert torch.equal(si, idx[p, :c].long()) and torch.equal(sd.view(-1), dist[p, :c])


def test_match_batch_stays_inside_its_buffers_over_any_workspace():
    """Every buffer of balf_match_smnn_batch at exactly its documented size between guard bands; the workspace filled with
    0x00, 0xFF (NaN) and 0xC0 bytes (-6.03: the one pattern that passes `ratio <= -1`, the threshold pairs with fewer than
    two rows get).  match_nn_kernel leaves rows >= n and whole pairs with an empty side unwritten: nothing may read them."""
    l = _lib.lib()
    P, K = 5, 300
    n1 = np.array([300, 257, 1, 64, 0], np.int32)
    n2 = np.array([300, 300, 200, 2, 100], np.int32)
    d1, d2 = _batch_descs(P, K, n1, n2, 8)
    g1, g2 = Guarded(P * K * 128 * 4, fill=0), Guarded(P * K * 128 * 4, fill=0)
    g1.view(torch.float32, (P, K, 128))[:] = torch.from_numpy(d1).to(DEV)
    g2.view(torch.float32, (P, K, 128))[:] = torch.from_numpy(d2).to(DEV)
    c1, c2 = Guarded(P * 4, fill=0), Guarded(P * 4, fill=0)
    c1.view(torch.int32, (P,))[:] = torch.from_numpy(n1).to(DEV)
    c2.view(torch.int32, (P,))[:] = torch.from_numpy(n2).to(DEV)
    nbytes = l.balf_match_smnn_batch_workspace_bytes(P, K, K)
    assert nbytes == 2 * ((P * K * 8 + 255) // 256 * 256)           # (nn index, ratio) per row, both directions
    outs = []
    for fill in (0x00, 0xFF, 0xC0):
        ws = Guarded(nbytes, fill=fill)
        idx, dist, count = Guarded(P * K * 2 * 4), Guarded(P * K * 4), Guarded(P * 4)
        rc = l.balf_match_smnn_batch(g1.ptr, K, c1.ptr, g2.ptr, K, c2.ptr, P, 0.95, idx.ptr, dist.ptr, count.ptr, ws.ptr,
                                     ws.n, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        for name, g in (("desc1", g1), ("desc2", g2), ("n1", c1), ("n2", c2), ("idx", idx), ("dist", dist),
                        ("count", count), ("workspace", ws)):
            assert g.intact(), f"balf_match_smnn_batch touched memory outside {name} (workspace fill {fill:#x})"
        outs.append((idx.view(torch.int32, (P, K, 2)).clone(), dist.view(torch.int32, (P, K)).clone(),
                     count.view(torch.int32, (P,)).clone()))
        assert l.balf_match_smnn_batch(g1.ptr, K, c1.ptr, g2.ptr, K, c2.ptr, P, 0.95, idx.ptr, dist.ptr, count.ptr, ws.ptr,
                                       ws.n - 1, _stream()) == ERR_WORKSPACE
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), "the result depends on what the workspace held"
    idx, dist, count = outs[0]
    dist = dist.view(torch.float32)
    assert int(count[2]) == 0 and int(count[4]) == 0 and min(count.tolist()[:2]) >= 100     # one row / no rows: no matches
    for p in range(P):
        c = int(count[p])
        assert bool((idx[p, c:] == -1).all()) and bool((dist[p, c:] == 0).all())
        if n1[p] and n2[p]:
            DC.MatchRef(d1[p, :n1[p]], d2[p, :n2[p]], 0.95).check(idx[p, :c].cpu().numpy(), dist[p, :c].cpu().numpy())


# ---- patches --------------------------------------------------------------------------------------------------------
# GPU against the fp64 reference: PATCH_GPU_FACTOR (4) x the measured discrepancy between the two references
# (1.262e-5 between the fp32 oracle and the fp64 restatement, recorded as 1.27e-5 in descriptor_common)
PATCH_TOL = DC.PATCH_GPU_FACTOR * DC.PATCH_F32_ORACLE_VS_F64


@pytest.mark.parametrize("h,w,scale,what", DC.PATCH_CASES)
def test_extract_patches_vs_fp64_reference(h, w, scale, what):
    """Every case kept: tests/test_descriptor_edges_host.py shows that the fp32 level formula of the library and the fp64
    one pick the same level for all of them, the two inputs either side of scale 32 included."""
    assert DC.level_f32(h, w, scale) == DC.level_f64(h, w, scale)
    gray, xy = DC.patch_image(h, w), DC.patch_points(h, w)
    ref = DC.extract_patches_f64(gray, xy, scale)
    got = ops.extract_patches(torch.from_numpy(gray).to(DEV), torch.from_numpy(xy).to(DEV), float(np.float32(scale)))
    assert got.shape == (DC.PATCH_POINTS, 1, 32, 32)
    err = float(np.abs(got.cpu().numpy()[:, 0].astype(np.float64) - ref).max())
    print(f"  {h}x{w} scale {scale!r} ({what}): max |GPU - fp64| = {err:.3e} (allowed {PATCH_TOL:.3e})")
    assert err <= PATCH_TOL


@pytest.mark.parametrize("h,w,scale,levels", [(160, 200, 300.0, 4), (480, 640, 12.0, 0)])
def test_extract_patches_batch_buffers_and_masking(h, w, scale, levels):
    """balf_extract_patches_batch through the C ABI: image, xy, count, patches and workspace between guard bands at the
    documented sizes.  160x200 at scale 300 asks for level 4 and makes 3 (the loop stops below the patch size): the
    workspace size and the launch loop have to agree there.  480x640 at scale 12 is level 0: the minimal workspace."""
    l = _lib.lib()
    B, K = 3, 40
    cnt = [40, 5, 0]
    nbytes = DC.patch_workspace_bytes(B, h, w, levels)              # the documented size, worked out here
    assert l.balf_extract_patches_batch_workspace_bytes(B, h, w, scale) == nbytes
    grays = np.stack([DC.patch_image(h + i, w)[:h] for i in range(B)])
    xy = np.stack([DC.patch_points(h, w, K) + np.float32(0.125 * i) for i in range(B)])
    img, pts, count = Guarded(B * h * w, fill=0), Guarded(B * K * 2 * 4, fill=0), Guarded(B * 4, fill=0)
    img.view(torch.uint8, (B, h, w))[:] = torch.from_numpy(grays).to(DEV)
    pts.view(torch.float32, (B, K, 2))[:] = torch.from_numpy(xy).to(DEV)
    count.view(torch.int32, (B,))[:] = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    outs = []
    for fill in (0x00, 0xFF):
        ws = Guarded(nbytes, fill=fill)
        out = Guarded(B * K * 1024 * 4, fill=0xFF)                  # NaN everywhere: every slot has to be written
        rc = l.balf_extract_patches_batch(img.ptr, B, h, w, pts.ptr, count.ptr, K, scale, out.ptr, ws.ptr, ws.n, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        for name, g in (("image", img), ("xy", pts), ("count", count), ("patches", out), ("workspace", ws)):
            assert g.intact(), f"balf_extract_patches_batch touched memory outside {name} (workspace fill {fill:#x})"
        outs.append(out.view(torch.int32, (B, K, 32, 32)).clone())
        assert l.balf_extract_patches_batch(img.ptr, B, h, w, pts.ptr, count.ptr, K, scale, out.ptr, ws.ptr, ws.n - 1,
                                            _stream()) == ERR_WORKSPACE
    assert torch.equal(outs[0], outs[1]), "the patches depend on what the workspace held"
    got = outs[0].view(torch.float32)
    for b in range(B):
        assert bool((outs[0][b, cnt[b]:] == 0).all())               # exact +0.0 in the slots past the count
        if cnt[b]:
            single = ops.extract_patches(torch.from_numpy(grays[b]).to(DEV), torch.from_numpy(xy[b, :cnt[b]]).to(DEV), scale)
            assert torch.equal(got[b, :cnt[b]], single[:, 0])


# ---- HardNet masked slots across the 4096-patch chunk ----------------------------------------------------------------
HN_B, HN_K = 5, 1000
# the first: image 4 straddles patch 4096, image 1 is fully masked (whole 128-patch FC tiles), image 2 has one used slot.
# the second: in the second chunk the mask of local patch l is count[4] at slot 96 + l; read at slot l of image 0 instead
# (the chunk offset forgotten) it would skip patches that are used.
HN_COUNTS = [[1000, 0, 1, 999, 1000], [5, 1000, 0, 999, 1000]]


@functools.lru_cache(maxsize=None)
def _hn_inputs():
    x = synth.synthetic_patches(HN_B * HN_K, 77)
    picks = set(range(4096 - 8, 4096 + 8))
    for count in HN_COUNTS:
        for b, c in enumerate(count):
            used = list(range(b * HN_K, b * HN_K + c))
            picks.update(used[:8] + used[-8:])
    picks = np.array(sorted(picks))
    sd64 = {k: v.double() for k, v in synth.synthetic_hardnet_state_dict(cases.HARDNET_SEED).items()}
    return x, picks, oracle.hardnet_forward(sd64, x[picks].double()).numpy()


@pytest.mark.parametrize("count", HN_COUNTS)
@pytest.mark.parametrize("precision,tol", [("fp16-split", DESC_TOL), ("fp16", 1e-3)])
def test_hardnet_masked_slots_across_the_chunk_boundary(precision, tol, count):
    x, picks, ref = _hn_inputs()
    m = HardNet()
    m.load_state_dict(synth.synthetic_hardnet_state_dict(cases.HARDNET_SEED))
    m.precision = precision
    m = m.eval().to(DEV)
    xg = x.to(DEV)
    with torch.inference_mode():
        full = m(xg)
        ws = ops._workspace("hardnet", xg.device, 1)
        ws.view(torch.float32)[: ws.numel() // 4].fill_(float("nan"))          # poison the scratch
        d = m.forward_slots(xg.view(HN_B, HN_K, 1, 32, 32), torch.tensor(count, dtype=torch.int32))
    assert d.shape == (HN_B, HN_K, 128) and not torch.isnan(d).any()
    full = full.view(HN_B, HN_K, 128)
    for b, c in enumerate(count):
        assert torch.equal(d[b, :c], full[b, :c]), f"used slots of image {b} differ from the unmasked run"
        assert bool((d[b, c:].view(torch.int32) == 0).all()), f"masked slots of image {b} are not exact zeros"
    used = np.array([p % HN_K < count[p // HN_K] for p in picks])
    err = float(np.abs(d.view(-1, 128)[picks[used]].cpu().numpy() - ref[used]).max())
    print(f"  {precision}, count {count}: {used.sum()} slots against the fp64 oracle, max-abs {err:.2e} (allowed {tol:.0e})")
    assert used.sum() >= 40 and err < tol


# ---- gray conversion above the 65536-block grid cap ------------------------------------------------------------------
def test_rgb_to_gray_above_the_grid_cap():
    """4097 x 4096 = 16,781,312 pixels, just past 65536 blocks x 256 threads: the grid-stride loop runs a second time."""
    h, w = 4097, 4096
    assert h * w > 65536 * 256
    rgb = np.random.default_rng(9).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    ref = torch.from_numpy(DC.gray_formula(rgb)).to(DEV)
    src = torch.from_numpy(rgb).to(DEV)
    assert torch.equal(ops.rgb_to_gray_u8(src), ref)
    out = Guarded(h * w, fill=0)
    assert _lib.lib().balf_rgb_to_gray(src.data_ptr(), h * w, out.ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert out.intact() and torch.equal(out.view(torch.uint8, (h, w)), ref)
