"""The resident XModem sender (include/fskhip_next.h: fskhip_xmodem_tx_*) without a device: every refusal the calls make before they
touch one, held to its code and to the whole fskhip_last_error() string, in the header's order -- null outputs first, the null
handle last."""
import ctypes as C

import numpy as np
import pytest

import xmodem_tx_ref as ref

OK, E_INVALID = 0, -1
HOST, DEVICE = "fskhip_xmodem_tx_poll_host", "fskhip_xmodem_tx_poll_device"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def test_create_refusals_in_order(L):
    out = C.c_void_p(0x77)
    refused(L, L.fskhip_xmodem_tx_create(None, 128, 10, C.byref(out)), E_INVALID, "fskhip_xmodem_tx_create: null argument")
    refused(L, L.fskhip_xmodem_tx_create(0x1000, 128, 10, None), E_INVALID, "fskhip_xmodem_tx_create: null argument")   # (a refused call follows no pointer)
    refused(L, L.fskhip_xmodem_tx_create(None, 0, 10, C.byref(out)), E_INVALID, "fskhip_xmodem_tx_create: null argument")   # the null comes first
    for bad in (0, 256, 1000):
        refused(L, L.fskhip_xmodem_tx_create(0x1000, bad, 10, C.byref(out)), E_INVALID, "fskhip_xmodem_tx_create: max_payload_size %d is not in 1..255" % bad)
    assert out.value == 0x77
    assert L.fskhip_xmodem_tx_destroy(None) == OK


def test_send_state_and_reset_refusals(L):
    offsets, data, mask = np.array([5, 3, 0], np.uint64), np.zeros(8, np.uint8), np.ones(2, np.uint8)
    refused(L, L.fskhip_xmodem_tx_send_host(None, mask.ctypes.data, None, data.ctypes.data), E_INVALID, "fskhip_xmodem_tx_send_host: null offsets")
    refused(L, L.fskhip_xmodem_tx_send_host(None, None, offsets.ctypes.data, None), E_INVALID, "null sender")   # decreasing offsets: not looked at
    words = np.full(4, 300, np.uint32)   # out-of-range words: the sender is missed first, they are not looked at
    W = words.ctypes.data
    refused(L, L.fskhip_xmodem_tx_state_set(None, W, W, W, W, W, W), E_INVALID, "null sender")
    refused(L, L.fskhip_xmodem_tx_state_get(None, W, None, None, None, None, None), E_INVALID, "null sender")
    refused(L, L.fskhip_xmodem_tx_reset(None, -1), E_INVALID, "null sender")
    refused(L, L.fskhip_xmodem_tx_reset(None, 1 << 40), E_INVALID, "null sender")
    assert (words == 300).all()


def test_host_form_refusals_in_order(L):
    call = L.fskhip_xmodem_tx_poll_host
    streams, events = np.zeros(4, np.uint32), np.zeros(4, ref.EVENT_DTYPE)
    ST, EV = streams.ctypes.data, events.ctypes.data
    ne = C.c_uint32(7)
    NE = C.addressof(ne)
    refused(L, call(None, None, None, ST, EV, 4, None), E_INVALID, HOST + ": null n_events")
    refused(L, call(None, None, None, None, None, 4, None), E_INVALID, HOST + ": null n_events")
    for st, ev in ((None, EV), (ST, None), (None, None)):
        refused(L, call(None, None, None, st, ev, 4, NE), E_INVALID, HOST + ": null streams or events with cap_streams 4")
    refused(L, call(None, None, None, ST, EV, 4, NE), E_INVALID, "null sender")
    refused(L, call(None, None, None, None, None, 0, NE), E_INVALID, "null sender")   # as the size query would be made
    assert ne.value == 7 and not streams.any() and not events["status"].any()   # a refused call writes nothing


def test_device_form_refusals_in_order(L):
    call = L.fskhip_xmodem_tx_poll_device
    MA, AB, ST, EV, TOT = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # (device pointers; a refused call never follows one)
    refused(L, call(None, MA, AB, ST, EV, 4, None, None), E_INVALID, DEVICE + ": null d_totals")
    for st, ev in ((None, EV), (ST, None)):
        refused(L, call(None, MA, AB, st, ev, 9, TOT, None), E_INVALID, DEVICE + ": null streams or events with cap_streams 9")
    refused(L, call(None, MA, AB, ST, EV, 9, TOT, None), E_INVALID, "null sender")
    refused(L, call(None, None, None, None, None, 0, TOT, 0x6000), E_INVALID, "null sender")
