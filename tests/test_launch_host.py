"""The one door into the library (balf_amd/_lib.py: on_device, launch) without a GPU: a recording stand-in for the
library, torch's device and stream accessors stubbed, CPU tensors (they have a ``data_ptr``)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from balf_amd import _lib
from balf_amd._lib import BalfHipError, Workspace, launch, on_device

REASON = "a made-up reason"


class RecordingLib:
    """What lib() returns here: one entry that records its arguments and the device that was current when it was called."""

    def __init__(self, state):
        self.state, self.calls, self.rc = state, [], 0

    def balf_probe(self, *args):
        self.calls.append((self.state.current, args))
        return self.rc

    def balf_error_string(self, rc):
        return f"{REASON} {rc}".encode()


def _raw(index):
    return 0x1000 + index


def _object_stream(index):
    return 0x2000 + index


@pytest.fixture
def door(monkeypatch):
    """Device 0 is current; ``state.entered`` lists the devices the context manager was entered for."""
    state = types.SimpleNamespace(current=0, entered=[])

    class Device:
        def __init__(self, index):
            self.index = index

        def __enter__(self):
            state.entered.append(self.index)
            self.before, state.current = state.current, self.index

        def __exit__(self, *exc):
            state.current = self.before

    monkeypatch.setattr(torch.cuda, "current_device", lambda: state.current)
    monkeypatch.setattr(torch.cuda, "device", Device)
    monkeypatch.setattr(torch._C, "_cuda_getCurrentRawStream", _raw, raising=False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda index: types.SimpleNamespace(cuda_stream=_object_stream(index)))
    state.lib = RecordingLib(state)
    monkeypatch.setattr(_lib, "_lib", state.lib)
    return state


def test_every_kind_of_argument_reaches_the_entry_in_its_place(door):
    x, y = torch.zeros(5), torch.zeros(3, dtype=torch.int32)
    ws = torch.empty(300, dtype=torch.uint8)
    array = (C.c_double * 2)(1.0, 2.0)
    host = np.zeros(9).ctypes.data_as(C.c_void_p)
    assert launch("balf_probe", 0, x, None, 7, Workspace(ws), 2.5, array, host, y) is None
    (device, args), = door.lib.calls
    assert device == 0
    assert args[:3] == (x.data_ptr(), None, 7)                      # a tensor -> its pointer, None -> NULL, a number as it is
    assert args[3:5] == (ws.data_ptr(), 300)                        # the workspace -> pointer and byte count, where it stood
    assert args[5] == 2.5 and type(args[5]) is float
    assert args[6] is array and args[7] is host                     # ctypes arrays and host pointers untouched
    assert args[8] == y.data_ptr()
    assert args[9:] == (_raw(0),)                                   # the stream last
    assert door.entered == []


def test_a_workspace_is_marked_never_guessed_from_its_dtype(door):
    ws = torch.empty(64, dtype=torch.uint8)
    launch("balf_probe", 0, ws, Workspace(ws))
    assert door.lib.calls[0][1] == (ws.data_ptr(), ws.data_ptr(), 64, _raw(0))


@pytest.mark.parametrize("dev", [0, torch.device("cuda", 0), torch.device("cuda")], ids=["index", "device", "no-index"])
def test_the_current_device_is_not_entered(door, dev):
    launch("balf_probe", dev, 1)
    assert door.entered == []
    assert door.lib.calls == [(0, (1, _raw(0)))]


@pytest.mark.parametrize("dev", [1, torch.device("cuda", 1)], ids=["index", "device"])
def test_another_device_is_entered_for_the_call_and_left_after_it(door, dev):
    launch("balf_probe", dev, 1)
    assert door.entered == [1]
    assert door.lib.calls == [(1, (1, _raw(1)))]                    # called with device 1 current, on device 1's stream
    assert door.current == 0
    door.current = 1                                                 # ... and once it is current, not entered again
    launch("balf_probe", dev, 2)
    assert door.entered == [1] and door.lib.calls[1] == (1, (2, _raw(1)))


@pytest.mark.parametrize("dev, entered", [(0, []), (1, [1])])
def test_without_the_raw_accessor_the_stream_comes_from_the_stream_object(door, monkeypatch, dev, entered):
    monkeypatch.delattr(torch._C, "_cuda_getCurrentRawStream")
    launch("balf_probe", dev, 1)
    assert door.lib.calls == [(dev, (1, _object_stream(dev)))]
    assert door.entered == entered


def test_the_low_layer_hands_back_what_the_call_returns(door):
    assert on_device(1, lambda stream: ("rc", stream)) == ("rc", _raw(1))
    assert on_device(0, lambda stream: ("rc", stream)) == ("rc", _raw(0))
    assert door.entered == [1]


def test_a_failure_is_reported_under_the_entry_s_name_or_the_given_label(door):
    door.lib.rc = 3
    with pytest.raises(BalfHipError) as e:
        launch("balf_probe", 0, 1)
    assert "balf_probe failed" in str(e.value) and f"{REASON} 3" in str(e.value)
    with pytest.raises(BalfHipError) as e:
        launch("balf_probe", 1, 1, what="balf_forward")
    assert "balf_forward failed" in str(e.value) and f"{REASON} 3" in str(e.value) and "balf_probe" not in str(e.value)
    assert door.current == 0                                         # the device is left on the way out of a failure too


def test_an_unknown_entry_is_refused(door):
    with pytest.raises(BalfHipError, match="balf_no_such_entry"):
        launch("balf_no_such_entry", 0, 1)
    assert door.lib.calls == []
