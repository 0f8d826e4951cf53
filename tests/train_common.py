"""What the reference modules of the training units (tests/*_train_common.py) share: the error measure of every gate, the
digest of the regenerated inputs, what a fixture records of a large result, and the slice geometry of the library's training
kernels restated (balf_amd/csrc/train_gemm.h: pixel_slices, and the three counts that a unit adds to it)."""
import hashlib

import numpy as np
import torch


# ---- the slice geometry, restated ---------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


MAX_SLICES = 64                             # kMaxSlices: slabs of a weight gradient
MAX_COL_PARTS = 1024                        # what PC stays at or below: col_rows = rows / 16 once that exceeds 64


def pixel_slices(n):
    """train_gemm.h: pixel_slices(N) -> (rows, S, col_rows, PC).  A weight gradient sums over the pixels in S slices of ``rows``
    pixels (256, or the multiple of 256 that keeps S at 64), a float64 column sum in PC workgroups of ``col_rows`` rows (64, or
    rows / 16, which keeps PC at 1024)."""
    rows = 256 * _ceil_div(_ceil_div(n, 256), MAX_SLICES)
    col_rows = rows // 16 if rows // 16 > 64 else 64
    return rows, _ceil_div(n, rows), col_rows, _ceil_div(n, col_rows)


def last_part(n, size):
    """The length of the last of the ceil(n / size) parts of ``n`` rows: in 1..size."""
    return n - (_ceil_div(n, size) - 1) * size


def head_row_partials(n):
    """head_train.hip: P, the partials per channel of the row kernels (1024 pixels per workgroup), channel-major [65][P]."""
    return _ceil_div(n, 1024)


def rcab_image_blocks(hw):
    """rcab_train.hip: (img_rows, PI), the PI row blocks of img_rows rows of ONE image of hw pixels in img_sum_kernel: 64 rows, or
    what keeps PI at 1024."""
    per = _ceil_div(hw, 1024)
    img_rows = per if per > 64 else 64
    return img_rows, _ceil_div(hw, img_rows)


def gmlp_mix_groups(n):
    """gmlp_train.hip: (groups, gpw, PW): the groups of 64 tokens, the groups per workgroup of mix_bwd_kernel (at most 256
    workgroups) and the workgroups."""
    groups = n // 64
    gpw = _ceil_div(groups, 256)
    return groups, gpw, _ceil_div(groups, gpw)


def linrelu_workspace_bytes(n, c_in):
    """linrelu_train.hip: make_layout: gm [N, 2c] float32, the column partials [PC, 2c] float64, the slabs [S, 2c, c] float32, each
    rounded up to 256 bytes."""
    _, s, _, pc = pixel_slices(n)
    al = lambda b: _ceil_div(b, 256) * 256                      # noqa: E731
    return al(n * 2 * c_in * 4) + al(pc * 2 * c_in * 8) + al(s * 2 * c_in * c_in * 4)


# The smallest shapes that reach the upper regimes of that geometry and meet each unit's shape rules: (B, Hc, Wc), for linrelu
# (N, c_in).  The GPU sweeps append them to their own; tests/test_train_geometry_host.py asserts what each is there for.
LARGE_SHAPES = {
    "head": ((1, 129, 131), (1, 257, 257)),
    "rcab": ((1, 129, 131), (2, 257, 257)),
    "gmlp": ((1, 8, 2056), (2, 216, 152)),
    "linrelu": ((16899, 128), (65536, 128), (65537, 32), (65537, 128)),
}


def to_device(case, device):
    """The tensors of a seeded case -- a tensor, a dict of them, tuples of either -- on ``device`` (None: as they are)."""
    if device is None:
        return case
    if isinstance(case, dict):
        return {k: to_device(v, device) for k, v in case.items()}
    if isinstance(case, (tuple, list)):
        return tuple(to_device(v, device) for v in case)
    return case.to(device)


def err(got, want64, scale):
    """max |got - want| / S, the measure of every gate."""
    want64 = torch.as_tensor(np.asarray(want64)).double() if not isinstance(want64, torch.Tensor) else want64.double()
    got = torch.as_tensor(np.asarray(got)) if not isinstance(got, torch.Tensor) else got.detach()
    got = got.double().to(want64.device)                # the difference is taken where the restatement lies
    return float((got.reshape(want64.shape) - want64).abs().max()) / scale


def composition_figures(what, composed, res, names, measure=err):
    """err(T) of the float32 torch-op composition's outputs ``composed`` (a unit's compose_f32 at the inputs of the case) in the
    scales of the restatement ``res``, printed next to the library's own: what any float32 implementation does at this shape.
    -> name -> figure."""
    figs = {k: measure(composed[k], res[k], res["S"][k]) for k in names if composed.get(k) is not None}
    print(what, "float32 composition:", " ".join(f"{k} {e:.2e}" for k, e in figs.items()))
    return figs


def inputs_digest(*tensors, keys=sorted):
    """SHA-256 over the float32 bytes of tensors, dicts (their values in the order ``keys(dict)``) and tuples of them: recorded
    next to the reference's results, so that a drift of a seeded generator or of synth.synthetic_state_dict -- which would
    silently pair new inputs with old results -- fails loudly instead."""
    h = hashlib.sha256()

    def feed(t):
        if isinstance(t, dict):
            for k in keys(t):
                feed(t[k])
        elif isinstance(t, (tuple, list)):
            for u in t:
                feed(u)
        else:
            h.update(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32)).tobytes())

    feed(tensors)
    return h.hexdigest()


def recorded_part(t, whole, every):
    """What a fixture records of a reference RESULT ``t``: all of it up to ``whole`` elements, else -- as a matrix of rows of
    its last axis -- rows 0..7 and every ``every``-th row.  A fixture must stay under 1 MB, and every output is checked whole
    against the float64 restatement anyway; d_T was taken on the whole results."""
    if t.numel() <= whole:
        return t
    rows = t.reshape(-1, t.shape[-1])
    return rows[sorted(set(range(8)) | set(range(0, rows.shape[0], every)))]


def recorded(fx, name, k, full, part):
    """-> (the reference's recorded float32 result, the same part of ``full``); ``part``: the module's recorded_part."""
    return torch.from_numpy(fx[f"{name}.{k}"]), part(full)
