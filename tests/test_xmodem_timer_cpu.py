"""The resident XModem wait timers without a GPU: the rule (csrc/fsk_xmodem_timer.h) walked together with the two transitions it
surrounds as a host program under ASan + UBSan (tests/cpp/xmodem_timer_check.cpp: scripted sequences with the flags and words
written out by hand), the refusals of the C ABI that need no device, in the order the checks are made, and the Python surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OK, E_INVALID = 0, -1
NAMES = ["fskhip_xmodem_timer_" + n for n in ("create_recv", "create_tx", "destroy", "reset", "state_get", "state_set")] + \
        ["fskhip_xmodem_%s_poll_timed_%s" % (k, f) for k in ("recv", "tx") for f in ("host", "device")]


def test_the_rule_as_a_host_program(tmp_path):
    exe = str(tmp_path / "xmodem_timer_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "xmodem_timer_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    last = r.stdout.splitlines()[-1].split()
    assert int(last[0]) >= 80 and last[1:] == ["expectations,", "0", "failed"], r.stdout


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, text):
    assert (rc, L.fskhip_last_error().decode()) == (E_INVALID, text)


def test_create_and_word_calls_refuse_before_any_device_call(L):
    out = C.c_void_p()
    fake = np.zeros(64, np.uint8)   # a non-null handle that must not be looked at
    for kind in ("recv", "tx"):
        fn = "fskhip_xmodem_timer_create_" + kind
        create = getattr(L, fn)
        refused(L, create(None, 144000, C.byref(out)), fn + ": null argument")
        refused(L, create(fake.ctypes.data, 144000, None), fn + ": null argument")
        refused(L, create(fake.ctypes.data, 0, C.byref(out)), fn + ": timeout_samples is 0")
    assert out.value is None and not fake.any()
    w = np.zeros(4, np.uint32)
    refused(L, L.fskhip_xmodem_timer_reset(None, -1), "fskhip_xmodem_timer_reset: null timer")
    refused(L, L.fskhip_xmodem_timer_state_get(None, w.ctypes.data, w.ctypes.data), "fskhip_xmodem_timer_state_get: null timer")
    refused(L, L.fskhip_xmodem_timer_state_set(None, w.ctypes.data, w.ctypes.data), "fskhip_xmodem_timer_state_set: null timer")
    assert L.fskhip_xmodem_timer_destroy(None) == OK


def test_timed_polls_refuse_in_the_plain_polls_order(L):
    ne, lists = C.c_uint32(7), np.zeros(64, np.uint32)
    P = lists.ctypes.data
    for kind in ("recv", "tx"):
        host, dev = "fskhip_xmodem_%s_poll_timed_host" % kind, "fskhip_xmodem_%s_poll_timed_device" % kind
        # the totals, then the lists, then the timer
        refused(L, getattr(L, host)(None, 128, None, None, None, None, 4, None), host + ": null n_events")
        refused(L, getattr(L, dev)(None, 128, None, None, None, None, 4, None, None), dev + ": null d_totals")
        refused(L, getattr(L, host)(None, 128, None, None, None, P, 4, C.byref(ne)), host + ": null streams or events with cap_streams 4")
        refused(L, getattr(L, host)(None, 128, None, None, P, None, 4, C.byref(ne)), host + ": null streams or events with cap_streams 4")
        refused(L, getattr(L, dev)(None, 128, None, None, None, P, 1, P, None), dev + ": null streams or events with cap_streams 1")
        refused(L, getattr(L, host)(None, 128, None, None, None, None, 0, C.byref(ne)), host + ": null timer")
        refused(L, getattr(L, host)(None, 128, None, None, P, P, 4, C.byref(ne)), host + ": null timer")
        refused(L, getattr(L, dev)(None, 128, None, None, None, None, 0, P, None), dev + ": null timer")
    assert ne.value == 7 and not lists.any()


def test_python_surface(L):
    import webaudio_modem_amd as wm
    from webaudio_modem_amd import _lib
    assert all(n in _lib.SYMBOL_NAMES and hasattr(L, n) for n in NAMES)
    cls = wm.XModemTimers
    assert all(callable(getattr(cls, m)) for m in ("from_ms", "poll", "poll_active", "state", "set_state", "reset", "close"))
    assert wm.xmodem.TIMER_WORDS == ("waited", "mark") and wm.xmodem.TIMER_WAS_PENDING == 4
    with pytest.raises(TypeError, match="needs an XModemFileReceiverBatch or an XModemSenderBatch"):
        cls(object())

    class Closed(wm.XModemFileReceiverBatch):
        def __init__(self):
            self._h, self.n_streams = None, 3
    with pytest.raises(ValueError, match="the handle has been closed"):
        cls(Closed())
    # timeoutMs in the engine's clock (3000 ms at 48 kHz), rounded up
    seen = []

    class Probe(cls):
        def __init__(self, handle, timeout_samples=144000):
            seen.append(timeout_samples)
    Probe.from_ms(None, 3000)
    Probe.from_ms(None, 1, sample_rate=44100)
    assert seen == [144000, 45]
    # the header speaks of the timers where the issue asks for it
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    assert "QUANTISED TO THE POLLS" in hdr and all(n in hdr for n in NAMES)
