"""What the chunked evaluation drivers share (``utils.train_utils``, ``benchmark_test.evaluate``): a chunk's
images and pairs, every image detected and described once in batches of one shape, the per-pair results read with ONE
device-to-host copy into a table with named columns, and the two retries on that read (``run_guarded``, ``with_edge_retry``)."""
import numpy as np
import torch

from .. import multiscale, ops
from ..guard import run_guarded
from ..pipeline import detect_batch, pad_image_on_device


def batches_by_shape(items, shape_of, batch_size):
    """Yield index lists: shapes (``shape_of(item)``) in first-seen order, input order within a shape, <= ``batch_size`` each."""
    groups = {}
    for i, item in enumerate(items):
        groups.setdefault(shape_of(item), []).append(i)
    for ids in groups.values():
        for b0 in range(0, len(ids), batch_size):
            yield ids[b0:b0 + batch_size]


def detection_rows(idx, score, count, w):
    """``detect_batch_u8``'s (idx [B,K] flat ``y * w + x``, score [B,K], count [B]) -> rows [B,K,4] float64 (x, y, 1.0, score);
    slots past an image's count are never read by the evaluation."""
    i = idx.to(torch.int64).clamp_(min=0)
    rows = torch.empty(idx.shape + (4,), dtype=torch.float64, device=idx.device)
    rows[..., 0] = i % w
    rows[..., 1] = torch.div(i, w, rounding_mode="floor")
    rows[..., 2] = 1.0
    rows[..., 3] = score
    return rows


def chunk_pairs(seqs):
    """The images of some sequences, each once, and their pairs in (sequence, destination) order -> (images, src_ids, dst_ids,
    hs, shapes): pair k is images[src_ids[k]] / images[dst_ids[k]] with h_dst_2_src hs[k] and shapes[k] = (h_src, w_src, h_dst,
    w_dst)."""
    images, src_ids, dst_ids, hs, shapes = [], [], [], [], []
    for sd in seqs:
        src = sd['im_src_RGB_norm']
        si = len(images)
        images.append(src)
        for k, im in enumerate(sd['images_dst_RGB_norm']):
            src_ids.append(si)
            dst_ids.append(len(images))
            images.append(im)
            hs.append(np.asarray(sd['h_dst_2_src'][k], dtype=np.float64).reshape(3, 3))
            shapes.append((src.shape[0], src.shape[1], im.shape[0], im.shape[1]))
    return images, src_ids, dst_ids, hs, shapes


def detect_images(images, model, device, nms_size, num_points, border_size, multi_scale, batch_size):
    """[H,W,3] float images on the host -> (rows [I,K,4] float64, count [I] int32) on the device: rows (x, y, radius, score)
    as ``extract_detections`` (radius 1.0) or ``extract_multiscale_detections`` returns them, rows past the count unused.
    Images of one shape go through the detector together, ``batch_size`` at a time (detection is batch-invariant)."""
    rows = torch.zeros((len(images), num_points, 4), dtype=torch.float64, device=device)
    count = torch.zeros((len(images),), dtype=torch.int32, device=device)
    for sel in batches_by_shape(images, lambda im: im.shape[:2], batch_size):
        at = torch.tensor(sel, dtype=torch.long, device=device)
        h, w = images[sel[0]].shape[:2]
        if multi_scale:
            x = torch.stack([torch.from_numpy(np.ascontiguousarray(images[i] if images[i].dtype in (np.float64, np.float32, np.float16)
                                                                   else images[i].astype(np.float64))).to(device)
                             for i in sel]).to(torch.float32)
            pts, cnt = multiscale.detect_batch_multiscale(model, x, num_points=num_points, border_size=border_size,
                                                          nms_size=nms_size)
            rows[at] = pts
        else:
            x = torch.cat([pad_image_on_device(images[i], device) for i in sel])
            idx, score, cnt, _ = detect_batch(model, x, h, w, border_size, nms_size, num_points)
            rows[at] = detection_rows(idx, score, cnt, w)
        count[at] = cnt
    return rows, count


def describe_images(grays, rows, count, descriptor, s_mult, batch_size):
    """One descriptor per detected row: gray images (device, [H,W] uint8 each), rows [I,K,4] / count [I] of
    :func:`detect_images` -> [I,K,128] float32 (zero rows past an image's count).  Images of one shape go through
    ``ops.extract_patches_batch`` and ``HardNet.forward_slots`` together, ``batch_size`` at a time."""
    desc = torch.zeros(rows.shape[:2] + (128,), dtype=torch.float32, device=rows.device)
    for sel in batches_by_shape(grays, lambda g: tuple(g.shape), batch_size):
        at = torch.tensor(sel, dtype=torch.long, device=rows.device)
        cnt = count[at]
        patches = ops.extract_patches_batch(torch.stack([grays[i] for i in sel]), rows[at][:, :, :2].float().contiguous(),
                                            cnt, float(s_mult))
        desc[at] = descriptor.forward_slots(patches, cnt)
    return desc


def pair_index(src_ids, dst_ids, device):      # (two long tensors on the device: gather per-image results per pair)
    return (torch.tensor(src_ids, dtype=torch.long, device=device), torch.tensor(dst_ids, dtype=torch.long, device=device))


# ---- the per-pair results of a chunk on the host ----------------------------------------------------------------------------------
class Table:
    """``values`` [..., C] float64 on the host with named columns: ``t[name]`` is the column, shaped ``values.shape[:-1]``.
    int32 fields make the trip int32 -> float64 -> ``int()``, which is exact."""

    def __init__(self, columns, values=None):
        self.columns = tuple(columns)
        self.values = np.zeros((0, len(self.columns))) if values is None else values

    def __getitem__(self, name):
        return self.values[..., self.columns.index(name)]


def stack_columns(result, fields, **extra):
    """The ``fields`` of a result NamedTuple of [P] device tensors, then the ``extra`` tensors, as float64 -> [P, C] on the device."""
    return torch.stack([getattr(result, k).double() for k in fields] + [v.double() for v in extra.values()], dim=1)


def host_table(result, fields, **extra):      # (the one device-to-host read of a chunk)
    return Table(fields + tuple(extra), stack_columns(result, fields, **extra).cpu().numpy())


def with_edge_retry(run):
    """``run()`` -> a :class:`Table` with ``compute_repeatability_batch``'s ``num_points_*`` / ``candidates_*`` columns.  A negative
    found count: some pair's candidates did not fit the default buffer; then ``run(max_edges=...)`` ONCE, sized from the totals
    (the larger of the two scales' sums over the pairs; values [P,L,C]: per leg, the largest leg; at least 1), as it comes."""
    t = run()
    if (t['num_points_single_scale'] < 0).any() or (t['num_points_multi_scale'] < 0).any():
        t = run(max_edges=int(max(t['candidates_single_scale'].sum(axis=0).max(), t['candidates_multi_scale'].sum(axis=0).max(), 1)))
    return t


def run_sequence_chunks(dataloader, model, chunk, columns, run_chunk):
    """The sequence drivers' loop: ``run_chunk(seqs)`` -> :class:`Table` per ``chunk`` sequences of ``dataloader`` under
    ``run_guarded`` -> (the names: ``sequence_name`` where the data has one, else ``sequences[i]``; one Table of all pairs)."""
    names, values = [], [Table(columns).values]
    n_seq = len(dataloader.sequences)
    for c0 in range(0, n_seq, chunk):
        seqs = [dataloader.get_sequence_data(i) for i in range(c0, min(n_seq, c0 + chunk))]
        names.extend(s['sequence_name'] if 'sequence_name' in s else dataloader.sequences[c0 + k] for k, s in enumerate(seqs))
        values.append(run_guarded(model, lambda: run_chunk(seqs)).values)
    return names, Table(columns, np.concatenate(values))
