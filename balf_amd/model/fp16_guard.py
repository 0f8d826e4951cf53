"""The per-call status blocks of the split-f16 forwards (include/balf_hip.h: balf_forward_status) and the three environment
switches of the split-f16 path.  ``Fp16Guard`` owns the rings, the pending calls and the looks; it neither launches nor
repairs: the module hands it a ``launch(status_ptr)`` per call and its one ``on_flag(pending, words, later)`` for a raised
word (``MLP_MA_DECODER._on_flag``: the verdict, the fp32 re-run and the warning text live there)."""
from __future__ import annotations

import collections
import os
import weakref

import torch

from .._lib import STATUS_WORDS

SLOTS = 8


def guard_mode() -> str:
    """BALF_FP16_GUARD = lazy (default) | sync | off.  lazy: the status block of a split-f16 forward is looked at when the
    NEXT forward of the module starts (or in fp16_guard_check()), never with a synchronisation on the hot path; sync: before
    the forward returns (one stream synchronisation per call, the flagged batch is re-run before anyone sees it); off: the
    kernels get no status block."""
    m = os.environ.get("BALF_FP16_GUARD", "lazy")
    if m not in ("lazy", "sync", "off"):
        raise ValueError(f"BALF_FP16_GUARD must be lazy, sync or off, got {m!r}")
    return m


def strict() -> bool:
    """BALF_FP16_STRICT=1: a checkpoint or a batch outside the range of the split-f16 path raises instead of falling back."""
    return os.environ.get("BALF_FP16_STRICT") == "1"


def check_enabled() -> bool:
    """BALF_FP16_CHECK=0 turns the load-time probes off (a verdict set by the guard holds all the same)."""
    return os.environ.get("BALF_FP16_CHECK", "1") != "0"


def _pinned_words(n: int) -> torch.Tensor:
    with torch.inference_mode(False):   # (a NORMAL tensor even when the first forward runs under torch.inference_mode(): an
        # inference tensor could not be cleared from outside that mode later)
        return torch.zeros(n, dtype=torch.int32).pin_memory()


# A guarded split-f16 forward that has not been looked at yet.  Holds NO tensor: scalars, an event recorded behind the call and
# weak references to its input and outputs, so that a batch the caller has dropped is freed at once (the closure
# kept here before pinned ~1.3 GB at 32 x 1080p until the next forward).  ``what``: the caller's own scalars, handed back to
# ``on_flag`` untouched.
_PendingCall = collections.namedtuple("_PendingCall", "ev device slot seq what refs")


class _Ring:
    """The status blocks of one device: a RING of SLOTS blocks of four ints in PINNED HOST memory.  Every guarded call gets a
    block of its own, so that a word raised by call A is attributed to A however far the host has run ahead (with one shared
    block a flag of A was charged to whatever call happened to be pending when the host looked); the kernels store
    into it when a softmax denominator is not finite or a stage output reaches the largest f16, the host reads it without a
    copy.  ``pending``: the calls not yet looked at, oldest first; ``seq``: the number of the last guarded call."""
    __slots__ = ("words", "pending", "seq")

    def __init__(self, words):
        self.words, self.pending, self.seq = words, collections.deque(), 0

    def ptr(self, slot: int) -> int:
        return self.words.data_ptr() + slot * STATUS_WORDS * 4

    def read_and_clear(self, slot: int):
        v = self.words[slot * STATUS_WORDS:(slot + 1) * STATUS_WORDS]
        w = v.tolist()
        if any(w):
            v.zero_()
        return w


class Fp16Guard:
    """One per module.  ``on_flag(pending, words, later)`` is called for every looked-at call whose block holds a word
    (``later``: how many calls were enqueued behind it); it returns True when it set the module's fp32 verdict, which
    ``switched`` counts.  It is an argument of every method that looks and is not kept: the guard holds no reference back to
    its module, so a dropped model is freed without waiting for the cycle collector.  ``new_words(n)`` / ``new_event()``: the
    status-word buffer and the event of a call (a test drives the state machine with a plain tensor and fake events)."""

    def __init__(self, new_words=_pinned_words, new_event=torch.cuda.Event):
        self._new_words, self._new_event = new_words, new_event
        self.rings = {}                # device -> _Ring
        self.switched = 0

    def submit(self, device, guarded, launch, on_flag, what, tensors) -> None:
        """Run one forward on ``device``: ``launch(status_ptr or None)`` enqueues it and returns the stream it went to;
        ``tensors`` = (input, prob, logits or None).  ``guarded``: a split-f16 forward outside validate_fp16 and outside graph
        capture.  Such a call gets a status block of its own for the kernels; what it says is acted on
        according to BALF_FP16_GUARD (see guard_mode): a flagged batch is re-run on the exact-fp32 kernels INTO THE SAME
        OUTPUT TENSORS, the module warns (BALF_FP16_STRICT=1: raises) and these weights run on the fp32 kernels from then on
        (effective_precision says so).  ``sync``: that happens before the forward returns -- nobody sees a flagged value.
        ``lazy`` (default): the look happens when a later forward starts (or in fp16_guard_check()), never with a wait on the
        hot path; the repair is stream-ordered, so GPU work enqueued AFTER it sees the repaired tensors, but what was enqueued
        between the flagged call and the look (the NMS of pipeline.detect_batch, a copy to the host) has used the split path's
        values: the warning names the call and says how many later ones had been enqueued -- repeat those, or run with
        BALF_FP16_GUARD=sync where that matters.  Only weak references are kept: outputs the caller has dropped are not
        repaired (and not kept alive)."""
        mode = guard_mode()
        if not guarded or mode == "off":
            launch(None)
            return
        r = self.rings.get(device)
        if r is None:
            r = self.rings[device] = _Ring(self._new_words(SLOTS * STATUS_WORDS))
        if len(r.pending) >= SLOTS:                              # the host is a whole ring ahead: the oldest call's block is
            r.pending[0].ev.synchronize()                        # needed again -- wait for that call (only) and look at it
            self._look(r, on_flag, final=False)
        slot = r.seq % SLOTS
        r.seq += 1
        stream = launch(r.ptr(slot))
        ev = self._new_event()
        ev.record(stream)
        refs = tuple(weakref.ref(t) if t is not None else None for t in tensors)
        r.pending.append(_PendingCall(ev, device, slot, r.seq, what, refs))
        if mode == "sync":
            ev.synchronize()
            self._look(r, on_flag, final=True)

    def look(self, device, on_flag, final: bool = False) -> None:
        r = self.rings.get(device)
        if r is not None and r.pending:
            self._look(r, on_flag, final)

    def _look(self, r, on_flag, final: bool) -> None:
        """Look at the status blocks of the pending calls the stream has passed, oldest first (``final``: it has passed all)."""
        while r.pending:
            p = r.pending[0]
            if not final and not p.ev.query():
                return                  # still running: its block is its own, a later look sees it
            r.pending.popleft()
            words = r.read_and_clear(p.slot)
            if any(words) and on_flag(p, words, len(r.pending)):
                self.switched += 1

    def check(self, on_flag, synchronize: bool = True) -> bool:
        """Look at every device's pending calls now (``synchronize``: wait for them first) -> whether a flag found by THESE
        looks set the fp32 verdict."""
        before = self.switched
        for r in self.rings.values():
            if r.pending and synchronize:
                r.pending[-1].ev.synchronize()
            self._look(r, on_flag, final=synchronize)
        return self.switched != before
