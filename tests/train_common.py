"""What the reference modules of the training units (tests/*_train_common.py) share: the error measure of every gate, the
digest of the regenerated inputs, and what a fixture records of a large result."""
import hashlib

import numpy as np
import torch


def err(got, want64, scale):
    """max |got - want| / S, the measure of every gate."""
    got = torch.as_tensor(np.asarray(got)).double() if not isinstance(got, torch.Tensor) else got.detach().double().cpu()
    want64 = torch.as_tensor(np.asarray(want64)).double() if not isinstance(want64, torch.Tensor) else want64.double()
    return float((got.reshape(want64.shape) - want64).abs().max()) / scale


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
