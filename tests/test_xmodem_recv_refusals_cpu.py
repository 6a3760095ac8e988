"""The resident XModem file receiver (include/fskhip_next.h: fskhip_xmodem_recv_*) without a device: every refusal the calls make
before they touch one, held to its code and to the whole fskhip_last_error() string, in the header's order -- null outputs first,
the null handle last."""
import ctypes as C

import numpy as np
import pytest

import xmodem_recv_ref as ref

OK, E_INVALID = 0, -1
HOST, DEVICE = "fskhip_xmodem_recv_poll_host", "fskhip_xmodem_recv_poll_device"
FILES, FILES_SET = "fskhip_xmodem_recv_files_host", "fskhip_xmodem_recv_files_set_host"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def test_create_refusals(L):
    out = C.c_void_p(0x77)
    refused(L, L.fskhip_xmodem_recv_create(None, 65536, 10, C.byref(out)), E_INVALID, "fskhip_xmodem_recv_create: null argument")
    refused(L, L.fskhip_xmodem_recv_create(0x1000, 65536, 10, None), E_INVALID, "fskhip_xmodem_recv_create: null argument")   # (a refused call follows no pointer)
    assert out.value == 0x77
    assert L.fskhip_xmodem_recv_destroy(None) == OK


def test_start_state_and_reset_refusals(L):
    mask = np.ones(2, np.uint8)
    refused(L, L.fskhip_xmodem_recv_start_host(None, mask.ctypes.data), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_recv_start_host(None, None), E_INVALID, "null receiver")
    words = np.full(4, 300, np.uint32)   # out-of-range words: the receiver is missed first, they are not looked at
    W = words.ctypes.data
    refused(L, L.fskhip_xmodem_recv_state_set(None, W, W, W, W, W, W, W), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_recv_state_get(None, W, None, None, None, None, None, None), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_recv_reset(None, -1), E_INVALID, "null receiver")
    refused(L, L.fskhip_xmodem_recv_reset(None, 1 << 40), E_INVALID, "null receiver")
    assert (words == 300).all()


def test_files_refusals_in_order(L):
    sel, offsets, data = np.array([900, 901], np.uint32), np.array([9, 5, 0], np.uint64), np.zeros(8, np.uint8)
    SEL, OFF, DATA = sel.ctypes.data, offsets.ctypes.data, data.ctypes.data
    nb = C.c_uint64(7)
    NB = C.addressof(nb)
    refused(L, L.fskhip_xmodem_recv_files_host(None, None, 2, None, None, 8, None), E_INVALID, FILES + ": null n_bytes")
    for s, o in ((None, OFF), (SEL, None)):
        refused(L, L.fskhip_xmodem_recv_files_host(None, s, 2, o, None, 8, NB), E_INVALID, FILES + ": null sel or offsets with n_sel 2")
    refused(L, L.fskhip_xmodem_recv_files_host(None, SEL, 2, OFF, None, 8, NB), E_INVALID, FILES + ": null data with cap_bytes 8")
    refused(L, L.fskhip_xmodem_recv_files_host(None, SEL, 2, OFF, DATA, 8, NB), E_INVALID, "null receiver")   # sel out of range: not looked at
    refused(L, L.fskhip_xmodem_recv_files_host(None, None, 0, None, None, 0, NB), E_INVALID, "null receiver")   # as the size query would be made
    assert nb.value == 7 and list(offsets) == [9, 5, 0] and not data.any()   # a refused call writes nothing
    for s, o in ((None, OFF), (SEL, None)):
        refused(L, L.fskhip_xmodem_recv_files_set_host(None, s, 2, o, DATA), E_INVALID, FILES_SET + ": null sel or offsets with n_sel 2")
    refused(L, L.fskhip_xmodem_recv_files_set_host(None, SEL, 2, OFF, None), E_INVALID, "null receiver")   # decreasing offsets, null data: not looked at
    refused(L, L.fskhip_xmodem_recv_files_set_host(None, None, 0, None, None), E_INVALID, "null receiver")


def test_host_form_refusals_in_order(L):
    call = L.fskhip_xmodem_recv_poll_host
    streams, events = np.zeros(4, np.uint32), np.zeros(4, ref.EVENT_DTYPE)
    ST, EV = streams.ctypes.data, events.ctypes.data
    ne = C.c_uint32(7)
    NE = C.addressof(ne)
    refused(L, call(None, None, None, None, ST, EV, 4, None), E_INVALID, HOST + ": null n_events")
    refused(L, call(None, None, None, None, None, None, 4, None), E_INVALID, HOST + ": null n_events")
    for st, ev in ((None, EV), (ST, None), (None, None)):
        refused(L, call(None, None, None, None, st, ev, 4, NE), E_INVALID, HOST + ": null streams or events with cap_streams 4")
    refused(L, call(None, None, None, None, ST, EV, 4, NE), E_INVALID, "null receiver")
    refused(L, call(None, None, None, None, None, None, 0, NE), E_INVALID, "null receiver")   # as the size query would be made
    assert ne.value == 7 and not streams.any() and not events["status"].any()   # a refused call writes nothing


def test_device_form_refusals_in_order(L):
    call = L.fskhip_xmodem_recv_poll_device
    MA, TO, AB, ST, EV, TOT = 0x1000, 0x1800, 0x2000, 0x3000, 0x4000, 0x5000   # (device pointers; a refused call never follows one)
    refused(L, call(None, MA, TO, AB, ST, EV, 4, None, None), E_INVALID, DEVICE + ": null d_totals")
    for st, ev in ((None, EV), (ST, None)):
        refused(L, call(None, MA, TO, AB, st, ev, 9, TOT, None), E_INVALID, DEVICE + ": null streams or events with cap_streams 9")
    refused(L, call(None, MA, TO, AB, ST, EV, 9, TOT, None), E_INVALID, "null receiver")
    refused(L, call(None, None, None, None, None, None, 0, TOT, 0x6000), E_INVALID, "null receiver")
