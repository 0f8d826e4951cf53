#!/usr/bin/env python3
"""The cost of the matching-score leg of the evaluation: evaluate.evaluate_matching_pairs for P pairs x N
points against its yardstick, evaluate.evaluate_pairs (the repeatability it sits beside) on the same inputs in the same run,
and against what a user writes without it: a loop of one-pair ops.match_smnn calls plus a NumPy verification.

Every number is named for what it is:
  *_eager_ms    host clock around `steps` calls that end in a device synchronise, per call (launch overhead included)
  *_graph_ms    device events around replays of the call captured with torch.cuda.graph, per replay: the device work alone
  part_*_ms     device events around eager calls of one library call, per call: an UPPER bound of the kernel's time (the gap
                between two eager launches is inside it); kernel times come from the kernel trace below
Every timed window holds `steps` calls (default 200: 0.5 s and more for the whole evaluation).
Usage: python tools/bench_matching.py [pairs=80] [points=1000] [steps=200] [out=profiles/matching_bench_p<pairs>_n<points>.json]
       rocprofv3 --kernel-trace --stats -d DIR -o matching -- python tools/bench_matching.py --core-only [pairs] [points] [calls=50]
       (--core-only: nothing but `calls` evaluate_matching_pairs calls after 3 warm-up calls, no timing, no file)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from balf_amd import ops                                               # noqa: E402
from balf_amd.benchmark_test import evaluate                           # noqa: E402

DEV = "cuda:0"
H, W = 480, 640


def make_inputs(p, n, seed=0):
    """P pairs of N detected rows in H x W images: the destination rows are the source rows in another order, moved by the
    pair's translation and up to 3 pixels of noise; their descriptors are the source's plus noise."""
    r = np.random.default_rng(seed)
    src = np.stack([r.integers(0, W, (p, n)), r.integers(0, H, (p, n)), np.ones((p, n)), r.uniform(0, 1, (p, n))],
                   axis=2).astype(np.float64)
    dst, hs, perms = np.empty_like(src), [], []
    for q in range(p):
        dx, dy = int(r.integers(-20, 21)), int(r.integers(-20, 21))
        hs.append(np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]]))
        perms.append(r.permutation(n))
        dst[q] = src[q, perms[q]]
        dst[q, :, 0] -= dx + r.integers(-3, 4, n)
        dst[q, :, 1] -= dy + r.integers(-3, 4, n)
    d_src = r.normal(0, 1, (p, n, 128)).astype(np.float32)
    d_src /= np.linalg.norm(d_src, axis=2, keepdims=True)
    d_dst = (np.stack([d_src[q, perms[q]] for q in range(p)]) + r.normal(0, 0.02, (p, n, 128))).astype(np.float32)
    cnt = np.full(p, n, dtype=np.int32)
    arrs = (src, cnt, d_src, dst, cnt.copy(), d_dst, np.stack(hs), np.array([[H, W, H, W]] * p, dtype=np.int32))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrs)


def eager_ms(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def events_ms(fn, steps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def graph_ms(fn, steps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fn()
    return events_ms(graph.replay, steps)


def user_loop_ms(src, ns, d_src, dst, nd, d_dst, h, shapes, thresholds):
    """What a user writes today, per pair: the one-pair matcher on the kept descriptors, the matches read back, the
    verification in NumPy.  (The kept lists themselves are taken from one batched filter call outside the timed loop.)"""
    cp = evaluate.common_points_index_batch(src, ns, dst, nd, h, shapes)
    kept = cp.kept.cpu().numpy()
    s_rows, d_rows = cp.src.cpu().numpy(), cp.dst_to_src.cpu().numpy()
    i_s, i_d = cp.src_index.long(), cp.dst_index.long()
    th = np.asarray(thresholds, dtype=np.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total = 0
    for q in range(src.shape[0]):
        ks, kd = int(kept[q, 0]), int(kept[q, 1])
        _, idx = ops.match_smnn(d_src[q][i_s[q, :ks]], d_dst[q][i_d[q, :kd]], 0.99)
        idx = idx.cpu().numpy()
        e = np.sqrt(((s_rows[q, idx[:, 0], :2] - d_rows[q, idx[:, 1], :2]) ** 2).sum(axis=1))
        total += int((e[:, None] <= th[None, :]).sum())
    return (time.perf_counter() - t0) * 1e3, total


def main():
    core_only = "--core-only" in sys.argv
    argv = [a for a in sys.argv if a != "--core-only"]
    p = int(argv[1]) if len(argv) > 1 else 80
    n = int(argv[2]) if len(argv) > 2 else 1000
    steps = int(argv[3]) if len(argv) > 3 else (50 if core_only else 200)
    if core_only:
        inputs = make_inputs(p, n)
        for _ in range(3 + steps):
            evaluate.evaluate_matching_pairs(*inputs)
        torch.cuda.synchronize()
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = argv[4] if len(argv) > 4 else os.path.join(root, "profiles", f"matching_bench_p{p}_n{n}.json")
    thresholds = list(range(1, 11))
    inputs = make_inputs(p, n)
    src, ns, d_src, dst, nd, d_dst, h, shapes = inputs
    rep_inputs = (src, ns, dst, nd, h, shapes)
    r = evaluate.evaluate_matching_pairs(*inputs)
    torch.cuda.synchronize()
    assert int(r.num_points_single_scale.min()) >= 0, "the default candidate buffer did not fit: fewer pairs or points"
    res = {"pairs": p, "points": n, "image": f"{W}x{H}", "steps": steps,
           "kept_mean": float(r.kept.double().mean()), "matches_mean": float(r.num_mutual_corresp.double().mean()),
           "mma_mean": float(r.mma.mean())}
    # alternate the two so that a drift of the machine hits both
    m_e, y_e, m_g, y_g = [], [], [], []
    for _ in range(3):
        m_e.append(eager_ms(lambda: evaluate.evaluate_matching_pairs(*inputs), steps))
        y_e.append(eager_ms(lambda: evaluate.evaluate_pairs(*rep_inputs), steps))
        m_g.append(graph_ms(lambda: evaluate.evaluate_matching_pairs(*inputs), steps))
        y_g.append(graph_ms(lambda: evaluate.evaluate_pairs(*rep_inputs), steps))
    res.update(matching_eager_ms=min(m_e), yardstick_eager_ms=min(y_e), matching_graph_ms=min(m_g), yardstick_graph_ms=min(y_g),
               matching_eager_all=m_e, yardstick_eager_all=y_e, matching_graph_all=m_g, yardstick_graph_all=y_g)
    res["ratio_eager"] = res["matching_eager_ms"] / res["yardstick_eager_ms"]
    res["ratio_graph"] = res["matching_graph_ms"] / res["yardstick_graph_ms"]
    cp = evaluate.common_points_index_batch(*rep_inputs)
    k_src = torch.gather(d_src, 1, cp.src_index.clamp(min=0).long().unsqueeze(2).expand(-1, -1, 128))
    k_dst = torch.gather(d_dst, 1, cp.dst_index.clamp(min=0).long().unsqueeze(2).expand(-1, -1, 128))
    _, midx, mcount = ops.match_smnn_batch(k_src, cp.kept[:, 0], k_dst, cp.kept[:, 1], 0.99)
    res["part_common_points_ms"] = events_ms(lambda: evaluate.common_points_batch(*rep_inputs), steps)
    res["part_common_points_index_ms"] = events_ms(lambda: evaluate.common_points_index_batch(*rep_inputs), steps)
    res["part_match_smnn_batch_ms"] = events_ms(lambda: ops.match_smnn_batch(k_src, cp.kept[:, 0], k_dst, cp.kept[:, 1], 0.99), steps)
    res["part_match_accuracy_ms"] = events_ms(
        lambda: evaluate.match_accuracy_batch(cp.src, cp.dst_to_src, cp.kept, midx, mcount, thresholds), steps)
    res["new_kernels_over_matcher"] = ((res["part_common_points_index_ms"] - res["part_common_points_ms"] +
                                        res["part_match_accuracy_ms"]) / res["part_match_smnn_batch_ms"])
    # bytes the verification moves per call: the match indices and both rows read, the error written
    m_total = int(mcount.sum())
    res["match_accuracy_bytes"] = m_total * (8 + 2 * 16) + p * midx.shape[1] * 8
    user_loop_ms(*inputs, thresholds)                                                          # warm-up
    loops = [user_loop_ms(*inputs, thresholds) for _ in range(3)]
    res["user_loop_ms"] = min(t for t, _ in loops)
    assert loops[0][1] == int(r.correct.sum()), (loops[0][1], int(r.correct.sum()))           # the same matches, the same counts
    res["user_loop_over_matching_eager"] = res["user_loop_ms"] / res["matching_eager_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
