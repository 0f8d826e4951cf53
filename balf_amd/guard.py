"""The one retry rule of every caller that consumes a split-f16 forward's results before the guard has looked at them
(``model/fp16_guard.py``).  Imports none of its callers."""


def run_guarded(model, run):
    """``run()`` -> its result, after the caller's device-to-host read has passed every forward ``run()`` enqueued: ``run``
    must END with that read (``int(count[0])`` of a one-image call, the ``.cpu()`` of a chunk's table), which makes the status
    blocks final, for free.  ``run()`` is repeated ONCE when the split-f16 guard finds a flag now
    (``fp16_guard_check(synchronize=False)``), or when the checkpoint was switched to the fp32 kernels while ``run()`` was in
    flight.  The second condition is not implied by the first: ``fp16_guard_check`` returns True only when THIS look finds a
    flag, and a ``run()`` of several forwards (a chunk, a pyramid) may have had a later forward look at an earlier one's status
    block already.  That look repairs ``prob``, switches the checkpoint and warns, but only after the flagged score map went
    into the NMS / selection enqueued behind it -- so a switch during ``run()`` repeats it just as a flag found now does.  The
    repeat runs on the fp32 kernels, which set no flag; its result is returned as it comes.  A model without
    ``fp16_guard_check`` (a plain ``nn.Module``, a stub) runs once."""
    guard = getattr(model, "fp16_guard_check", None)
    on_fp32 = getattr(model, "effective_precision", None) == "fp32"
    out = run()
    if guard is not None and (guard(synchronize=False) or (not on_fp32 and getattr(model, "effective_precision", None) == "fp32")):
        out = run()
    return out
