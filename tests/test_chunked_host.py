"""The shared pieces of the chunked evaluation drivers on stubs (no GPU, no library): the one guard retry
(``guard.run_guarded``) and the helpers of ``benchmark_test._chunked``."""
from typing import NamedTuple

import numpy as np
import torch

from balf_amd.benchmark_test import _chunked
from balf_amd.guard import run_guarded


# ---- run_guarded ------------------------------------------------------------------------------------------------------------------
class _Model:
    """``fp16_guard_check`` answers the scripted ``flags`` in turn; ``switch_during_run`` = the number of the run during which
    an earlier look (not this one) moves the checkpoint to the fp32 kernels."""

    def __init__(self, flags=(), precision="fp16", switch_during_run=None):
        self.flags, self.effective_precision, self.switch_during_run = list(flags), precision, switch_during_run
        self.runs, self.guard_calls = 0, []

    def fp16_guard_check(self, synchronize=True):
        self.guard_calls.append(synchronize)
        hit = self.flags.pop(0) if self.flags else False
        if hit:
            self.effective_precision = "fp32"
        return hit

    def run(self):
        self.runs += 1
        if self.runs == self.switch_during_run:
            self.effective_precision = "fp32"
        return f"run {self.runs}"


def test_run_guarded_without_guard_attributes_runs_once():
    calls = []
    assert run_guarded(object(), lambda: calls.append(1) or "x") == "x" and calls == [1]
    assert run_guarded(torch.nn.Linear(1, 1), lambda: calls.append(2) or "y") == "y" and calls == [1, 2]


def test_run_guarded_calm_runs_once():
    m = _Model()
    assert run_guarded(m, m.run) == "run 1" and m.runs == 1
    assert m.guard_calls == [False]                             # synchronize=False: the caller's read was the wait


def test_run_guarded_repeats_when_a_flag_is_found():
    m = _Model(flags=[True])
    assert run_guarded(m, m.run) == "run 2" and m.runs == 2     # the last run's value
    assert m.guard_calls == [False]


def test_run_guarded_repeats_when_the_checkpoint_was_switched_during_the_run():
    """The guard finds nothing NOW, but a later forward of the run has already acted on an earlier one's flag."""
    m = _Model(flags=[False], switch_during_run=1)
    assert run_guarded(m, m.run) == "run 2" and m.runs == 2
    assert m.effective_precision == "fp32" and m.guard_calls == [False]


def test_run_guarded_on_fp32_before_runs_once():
    m = _Model(precision="fp32")
    assert run_guarded(m, m.run) == "run 1" and m.runs == 1


def test_run_guarded_never_runs_a_third_time():
    m = _Model(flags=[True, True, True])
    assert run_guarded(m, m.run) == "run 2" and m.runs == 2 and m.guard_calls == [False]
    m = _Model(flags=[True], switch_during_run=2)
    assert run_guarded(m, m.run) == "run 2" and m.runs == 2


# ---- with_edge_retry ----------------------------------------------------------------------------------------------------------------
_EDGE = ('num_points_single_scale', 'num_points_multi_scale', 'candidates_single_scale', 'candidates_multi_scale')


def _edge_runs(*tables):
    """A ``run`` answering ``tables`` in turn (values [..., 4] in the order of _EDGE), and the list of its keyword arguments."""
    seen, left = [], [_chunked.Table(_EDGE, np.asarray(v, dtype=np.float64)) for v in tables]

    def run(**kw):
        seen.append(kw)
        return left.pop(0)
    return run, seen


def test_edge_retry_leaves_a_chunk_that_fits_alone():
    run, seen = _edge_runs([[3, 4, 10, 20], [0, 0, 5, 5]])
    t = _chunked.with_edge_retry(run)
    assert seen == [{}] and t['candidates_multi_scale'].tolist() == [20, 5]


def test_edge_retry_sizes_the_buffer_from_the_larger_total():
    for first, want in (([[-1, 4, 10, 20], [2, 2, 5, 6]], 26),          # single scale overflowed, the multi-scale sum is larger
                        ([[3, -1, 30, 20], [2, 2, 5, 6]], 35),          # multi scale overflowed, the single-scale sum is larger
                        ([[-1, -1, 0, 0], [0, 0, 0, 0]], 1)):           # no candidates at all: at least 1
        second = [[-1, -1, 1, 1], [1, 1, 1, 1]]                          # still negative: returned as it comes, no third run
        run, seen = _edge_runs(first, second)
        t = _chunked.with_edge_retry(run)
        assert seen == [{}, {"max_edges": want}] and type(seen[1]["max_edges"]) is int
        assert t.values.tolist() == second


def test_edge_retry_takes_the_maximum_over_the_legs():
    """Values [P, 2, C]: the validation's two legs per pair; the sums are per leg."""
    first = [[[1, 1, 10, 11], [-1, 1, 40, 2]],
             [[1, 1, 10, 11], [1, 1, 40, 2]]]                            # leg sums: single (20, 80), multi (22, 4)
    run, seen = _edge_runs(first, first)
    _chunked.with_edge_retry(run)
    assert seen == [{}, {"max_edges": 80}]


# ---- batches_by_shape ---------------------------------------------------------------------------------------------------------------
def test_batches_by_shape():
    items = [np.zeros(s) for s in ((4, 5), (2, 2), (4, 5), (4, 5), (2, 2), (4, 5), (7, 1), (4, 5))]
    got = list(_chunked.batches_by_shape(items, lambda a: a.shape, 2))
    assert got == [[0, 2], [3, 5], [7], [1, 4], [6]]            # first-seen shape order, input order within, the last one short
    assert list(_chunked.batches_by_shape(items, lambda a: a.shape, 1)) == [[0], [2], [3], [5], [7], [1], [4], [6]]
    assert list(_chunked.batches_by_shape(items, lambda a: a.shape, 100)) == [[0, 2, 3, 5, 7], [1, 4], [6]]
    assert list(_chunked.batches_by_shape([], lambda a: a.shape, 4)) == []


# ---- the named table ----------------------------------------------------------------------------------------------------------------
class _Result(NamedTuple):
    ratio: torch.Tensor
    found: torch.Tensor
    unused: torch.Tensor
    kept: torch.Tensor


def test_host_table_addresses_columns_by_name():
    big = 2 ** 31 - 1
    r = _Result(torch.tensor([0.1, float("nan"), -0.0], dtype=torch.float64), torch.tensor([big, -1, big - 1], dtype=torch.int32),
                torch.tensor([9, 9, 9], dtype=torch.int32), torch.tensor([[1, 2], [3, 4], [big, 0]], dtype=torch.int32))
    t = _chunked.host_table(r, ('found', 'ratio'), kept_src=r.kept[:, 0], kept_dst=r.kept[:, 1])
    assert t.columns == ('found', 'ratio', 'kept_src', 'kept_dst') and t.values.shape == (3, 4) and t.values.dtype == np.float64
    assert [int(v) for v in t['found']] == [big, -1, big - 1]                  # int32 -> float64 -> int() is exact
    assert [int(v) for v in t['kept_src']] == [1, 3, big] and [int(v) for v in t['kept_dst']] == [2, 4, 0]
    assert np.array_equal(t['ratio'].view(np.uint64), r.ratio.numpy().view(np.uint64))      # bits kept, NaN and -0.0 too
    stacked = _chunked.stack_columns(r, ('ratio', 'found'))
    assert stacked.dtype == torch.float64 and tuple(stacked.shape) == (3, 2) and np.isnan(stacked[1, 0].item())


def test_table_with_legs_and_empty_table():
    t = _chunked.Table(('a', 'b'), np.arange(12, dtype=np.float64).reshape(3, 2, 2))
    assert t['b'].shape == (3, 2) and t['b'][:, 1].tolist() == [3.0, 7.0, 11.0] and t['a'][-1, 0] == 8.0
    e = _chunked.Table(('a', 'b', 'c'))
    assert e.values.shape == (0, 3) and e['c'].shape == (0,)
