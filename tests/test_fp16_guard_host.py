"""The state machine of the split-f16 status-block guard (balf_amd/model/fp16_guard.py) on the host alone: fake events with a
settable ``query()`` and a counting ``synchronize()``, a plain int32 tensor for the status words, a recording ``launch`` and
``on_flag``.  No GPU and no library."""
import gc

import pytest
import torch

from balf_amd._lib import STATUS_WORDS
from balf_amd.model import fp16_guard
from balf_amd.model.fp16_guard import SLOTS, Fp16Guard

DEV = "dev0"


class FakeEvent:
    def __init__(self):
        self.done, self.syncs, self.stream = False, 0, None

    def record(self, stream):
        self.stream = stream

    def query(self):
        return self.done

    def synchronize(self):
        self.syncs += 1
        self.done = True


class Harness:
    """A guard on fakes.  ``submit()`` -> the pointer its launch got; ``flags``: (seq, words, later, refs alive) per on_flag."""

    def __init__(self, sets_verdict=True):
        self.events, self.launched, self.flags, self.log = [], [], [], []
        self.sets_verdict = sets_verdict
        self.guard = Fp16Guard(new_words=lambda n: torch.zeros(n, dtype=torch.int32), new_event=self._event)

    def _event(self):
        self.events.append(FakeEvent())
        return self.events[-1]

    def on_flag(self, p, words, later):
        self.log.append("flag")
        self.flags.append((p.seq, words, later, tuple(r() if r is not None else None for r in p.refs), p.what))
        return self.sets_verdict

    def launch(self, status):
        self.log.append("launch")
        self.launched.append(status)
        return "stream"

    def submit(self, guarded=True, tensors=(None, None, None), what=None):
        self.guard.submit(DEV, guarded, self.launch, self.on_flag, what, tensors)
        return self.launched[-1]

    @property
    def ring(self):
        return self.guard.rings[DEV]

    def raise_word(self, seq, word=1, value=1):
        self.ring.words[((seq - 1) % SLOTS) * STATUS_WORDS + word] = value


@pytest.fixture(autouse=True)
def lazy(monkeypatch):
    monkeypatch.delenv("BALF_FP16_GUARD", raising=False)


def test_slots_wrap_seq_counts_from_one_and_each_call_has_its_own_block():
    h = Harness()
    ptrs = []
    for i in range(2 * SLOTS + 1):
        ptrs.append(h.submit())
        p = h.ring.pending[-1]
        assert (p.seq, p.slot, p.device) == (i + 1, i % SLOTS, DEV) and h.ring.seq == i + 1
        assert p.ev is h.events[-1] and p.ev.stream == "stream"          # recorded behind the launch, on its stream
        h.events[-1].done = True
        h.guard.look(DEV, h.on_flag)                                     # (keeps the ring short: slots follow seq, not the queue)
    base = h.ring.words.data_ptr()
    assert ptrs == [base + (i % SLOTS) * STATUS_WORDS * 4 for i in range(2 * SLOTS + 1)]
    assert SLOTS == 8 and not h.flags


def test_a_full_ring_waits_for_the_oldest_call_only_before_the_next_launch():
    h = Harness()
    for _ in range(SLOTS):
        h.submit()
        assert len(h.ring.pending) <= SLOTS
    assert [e.syncs for e in h.events] == [0] * SLOTS
    h.raise_word(1)                                                      # call 1's block: its look must precede launch 9
    h.log.clear()
    ptr = h.submit()
    assert [e.syncs for e in h.events] == [1] + [0] * SLOTS              # one wait, on call 1's event
    assert h.log == ["flag", "launch"] and h.flags[0][0] == 1 and h.flags[0][2] == SLOTS - 1
    assert ptr == h.ring.ptr(0) and [p.seq for p in h.ring.pending] == list(range(2, SLOTS + 2))
    assert len(h.ring.pending) == SLOTS


def test_a_look_stops_at_the_first_unfinished_call():
    h = Harness()
    for _ in range(4):
        h.submit()
    h.raise_word(2, word=0, value=3)
    h.events[1].done = True                                              # call 2 finished, call 1 did not
    h.guard.look(DEV, h.on_flag)
    assert not h.flags and len(h.ring.pending) == 4
    assert not h.guard.check(h.on_flag, synchronize=False) and not h.flags
    h.events[0].done = True
    h.guard.look(DEV, h.on_flag)
    assert [(f[0], f[1], f[2]) for f in h.flags] == [(2, [3, 0, 0, 0], 2)]          # charged to call 2; calls 3, 4 behind it
    assert [p.seq for p in h.ring.pending] == [3, 4] and [e.syncs for e in h.events] == [0] * 4


def test_a_final_look_drains_and_clears_only_what_was_raised():
    h = Harness()
    for _ in range(5):
        h.submit()
    h.guard.look(DEV, h.on_flag, final=True)
    assert not h.ring.pending and not h.flags
    for _ in range(5):
        h.submit()                                                       # calls 6..10: slots 5, 6, 7, 0, 1
    h.raise_word(7, word=1)
    h.raise_word(9, word=2, value=5)
    version = h.ring.words._version
    assert h.guard.check(h.on_flag, synchronize=True)
    assert [e.syncs for e in h.events[5:]] == [0, 0, 0, 0, 1]            # check waits for the newest call, then drains
    assert [(f[0], f[1], f[2]) for f in h.flags] == [(7, [0, 1, 0, 0], 3), (9, [0, 0, 5, 0], 1)]
    assert not h.ring.pending and not h.ring.words.any()
    assert h.ring.words._version == version + 2                          # two blocks cleared, the other three not written
    assert not h.guard.check(h.on_flag, synchronize=True)


def test_sync_mode_acts_before_submit_returns(monkeypatch):
    monkeypatch.setenv("BALF_FP16_GUARD", "sync")
    h = Harness()
    h.submit()
    assert h.events[0].syncs == 1 and not h.ring.pending and not h.flags

    def launch(status):
        h.ring.words[(status - h.ring.words.data_ptr()) // 4 + 1] = 1    # the kernels raise RANGE in the block they were given
        return h.launch(status)
    h.guard.submit(DEV, True, launch, h.on_flag, None, (None, None, None))
    assert h.log == ["launch", "launch", "flag"] and h.flags[0][:3] == (2, [0, 1, 0, 0], 0)
    assert not h.ring.pending and h.guard.switched == 1


def test_off_mode_and_unguarded_calls_get_no_status_block(monkeypatch):
    h = Harness()
    assert h.submit(guarded=False) is None                               # fp32, validate_fp16, graph capture
    assert not h.guard.rings and not h.events
    monkeypatch.setenv("BALF_FP16_GUARD", "off")
    assert h.submit() is None and not h.guard.rings and not h.events
    monkeypatch.setenv("BALF_FP16_GUARD", "sometimes")
    with pytest.raises(ValueError, match="BALF_FP16_GUARD must be lazy, sync or off"):
        h.submit()
    h.guard.look(DEV, h.on_flag)                                         # a device without a ring: nothing to look at
    assert not h.guard.check(h.on_flag)


def test_a_pending_call_keeps_its_tensors_alive_only_weakly():
    h = Harness()
    src, prob = torch.zeros(3), torch.zeros(2)
    h.submit(tensors=(src, prob, None), what=("key", "f32"))
    refs = h.ring.pending[0].refs
    assert refs[0]() is src and refs[1]() is prob and refs[2] is None
    del prob
    gc.collect()
    assert refs[1]() is None
    h.raise_word(1)
    assert h.guard.check(h.on_flag)
    seq, _, later, alive, what = h.flags[0]
    assert (seq, later, what) == (1, 0, ("key", "f32")) and alive[0] is src and alive[1] is None and alive[2] is None


def test_check_reports_only_a_verdict_set_during_its_own_looks():
    h = Harness(sets_verdict=False)                                      # the weights changed since: acted on, no verdict
    h.submit()
    h.raise_word(1)
    assert not h.guard.check(h.on_flag) and len(h.flags) == 1 and h.guard.switched == 0
    h.sets_verdict = True
    h.submit()
    h.raise_word(2)
    h.events[1].done = True
    h.guard.look(DEV, h.on_flag)                                         # a later forward's look finds it first ...
    assert h.guard.switched == 1 and len(h.flags) == 2
    assert not h.guard.check(h.on_flag)                                  # ... so this check has nothing to report
    h.submit()
    h.raise_word(3)
    assert h.guard.check(h.on_flag) and h.guard.switched == 2


def test_the_three_switches_are_read_at_call_time(monkeypatch):
    for name in ("BALF_FP16_GUARD", "BALF_FP16_STRICT", "BALF_FP16_CHECK"):
        monkeypatch.delenv(name, raising=False)
    assert (fp16_guard.guard_mode(), fp16_guard.strict(), fp16_guard.check_enabled()) == ("lazy", False, True)
    monkeypatch.setenv("BALF_FP16_GUARD", "sync")
    monkeypatch.setenv("BALF_FP16_STRICT", "1")
    monkeypatch.setenv("BALF_FP16_CHECK", "0")
    assert (fp16_guard.guard_mode(), fp16_guard.strict(), fp16_guard.check_enabled()) == ("sync", True, False)
