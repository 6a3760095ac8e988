"""The compacted RX drain (include/fskhip_next.h: fskhip_processor_rx_drain_sparse_host / _device) without a device: every
refusal the two calls make before they touch one, held to its code and to the whole fskhip_last_error() string through ctypes,
in the order the header gives; and the image-building helper of the GPU tests (tests/drain_ref.py) -- its checksum and layout
against fskhip_processor_snapshot_info_get, which validates an image on the host."""
import ctypes as C

import numpy as np
import pytest

import drain_ref

OK, E_INVALID = 0, -1
HOST, DEVICE = "fskhip_processor_rx_drain_sparse_host", "fskhip_processor_rx_drain_sparse_device"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def test_host_form_refusals_in_order(L):
    call = L.fskhip_processor_rx_drain_sparse_host
    streams, offsets, data = np.zeros(4, np.uint32), np.zeros(5, np.uint32), np.zeros(64, np.uint8)
    ST, OF, DA = streams.ctypes.data, offsets.ctypes.data, data.ctypes.data
    na, nb = C.c_uint32(7), C.c_uint32(7)
    NA, NB = C.addressof(na), C.addressof(nb)
    # the totals first: without them not even a size can be reported
    for a, b in ((None, NB), (NA, None), (None, None)):
        refused(L, call(None, None, 1, ST, OF, 4, DA, 64, a, b), E_INVALID, HOST + ": null n_active or n_bytes")
    # a list that is missing although its cap says it has room
    for st, of in ((None, OF), (ST, None), (None, None)):
        refused(L, call(None, None, 1, st, of, 4, DA, 64, NA, NB), E_INVALID, HOST + ": null streams or offsets with cap_streams 4")
    refused(L, call(None, None, 1, ST, OF, 4, None, 64, NA, NB), E_INVALID, HOST + ": null data with cap_bytes 64")
    refused(L, call(None, None, 1, None, None, 0, None, 3, NA, NB), E_INVALID, HOST + ": null data with cap_bytes 3")
    # then the processor: with full lists, and as the size query (both caps 0, null lists) would be made
    refused(L, call(None, None, 1, ST, OF, 4, DA, 64, NA, NB), E_INVALID, "null processor")
    refused(L, call(None, None, 0, None, None, 0, None, 0, NA, NB), E_INVALID, "null processor")
    assert (na.value, nb.value) == (7, 7) and not streams.any() and not offsets.any() and not data.any()   # a refused call writes nothing


def test_device_form_refusals_in_order(L):
    call = L.fskhip_processor_rx_drain_sparse_device
    # (the pointers would be device pointers; a refused call never follows one)
    ST, OF, DA, TOT = 0x1000, 0x2000, 0x3000, 0x4000
    refused(L, call(None, None, 1, ST, OF, 4, DA, 64, None, None), E_INVALID, DEVICE + ": null d_totals")
    for st, of in ((None, OF), (ST, None)):
        refused(L, call(None, None, 1, st, of, 9, DA, 64, TOT, None), E_INVALID, DEVICE + ": null streams or offsets with cap_streams 9")
    refused(L, call(None, None, 1, ST, OF, 9, None, 1, TOT, None), E_INVALID, DEVICE + ": null data with cap_bytes 1")
    refused(L, call(None, None, 1, ST, OF, 9, DA, 64, TOT, None), E_INVALID, "null processor")
    refused(L, call(None, None, 5, None, None, 0, None, 0, TOT, 0x5000), E_INVALID, "null processor")


def test_symbols_are_in_the_python_table(L):
    from webaudio_modem_amd import _lib
    assert HOST in _lib.SYMBOL_NAMES and DEVICE in _lib.SYMBOL_NAMES
    from webaudio_modem_amd.processor import FSKProcessorBatch
    assert callable(FSKProcessorBatch.demodulate_sparse) and callable(FSKProcessorBatch.demodulate_active)


def info_of(L, image):
    from webaudio_modem_amd import _lib
    buf = np.frombuffer(bytes(image), np.uint8)
    info = _lib.ProcessorSnapshotInfo()
    rc = L.fskhip_processor_snapshot_info_get(buf.ctypes.data, buf.nbytes, C.byref(info))
    return rc, L.fskhip_last_error().decode(), info


@pytest.mark.parametrize("n_streams,cap", [(1, 1), (3, 16), (5, 100), (2, 1024)])
def test_helper_images_validate_on_the_host(L, n_streams, cap):
    """a hand-made image -- known words, known bytes -- passes the library's validation (magic, sizes, checksum, ring words)"""
    r = np.arange(n_streams) % cap
    n = (np.arange(n_streams) * 7 + 1) % (cap + 1)
    ring = (np.arange(n_streams * cap).reshape(n_streams, cap) % 255 + 1).astype(np.uint8)
    rings = drain_ref.Rings(r, n, ring)
    image = rings.image()
    rc, text, info = info_of(L, image)
    assert rc == OK, text
    rec = 64 + ((cap + 15) & ~15)
    assert (info.n_streams, info.rx_capacity, info.payload_capacity, info.record_bytes) == (n_streams, cap, 0, rec)
    assert len(image) == 48 + n_streams * rec
    # the layout by hand for the last stream: writeIndex | readIndex | _length, and the ring with zeros outside the live span
    s = n_streams - 1
    record = np.frombuffer(image, np.uint8)[48 + s * rec:48 + (s + 1) * rec]
    assert list(record[:16].view("<u4")) == [(r[s] + n[s]) % cap, r[s], n[s], 0]
    want = np.zeros(cap, np.uint8)
    for k in range(n[s]):
        want[(r[s] + k) % cap] = ring[s, (r[s] + k) % cap]
    assert np.array_equal(record[64:64 + cap], want) and not record[16:64].any() and not record[64 + cap:].any()
    # one flipped ring byte, or a checksum computed any other way, is refused by name
    bad = bytearray(image)
    bad[48 + 64] ^= 0x01   # (record 0's first ring byte)
    rc, text, _ = info_of(L, bad)
    assert rc == E_INVALID and "checksum" in text, text


def test_helper_checksum_is_the_sequential_formula():
    """drain_ref.checksum sums in closed form; here the header's two running sums, word by word"""
    image = np.frombuffer(drain_ref.Rings([2, 0], [3, 4], np.arange(1, 9, dtype=np.uint8).reshape(2, 4)).image(), np.uint8).copy()
    stored = int(image[32:40].view("<u8")[0])
    image[32:40] = 0
    a = b = 0
    for w in image.view("<u8"):
        a = (a + int(w)) & (2**64 - 1)
        b = (b + a) & (2**64 - 1)
    assert stored == ((a * 0x9E3779B97F4A7C15) & (2**64 - 1)) ^ b


def test_helper_expectation_on_a_hand_made_state():
    """the numpy drain itself on a state small enough to write down"""
    ring = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]], np.uint8)
    rings = drain_ref.Rings([3, 0, 1, 2], [2, 0, 4, 1], ring)
    streams, offsets, data, after = rings.drained()
    assert list(streams) == [0, 2, 3] and list(offsets) == [0, 2, 6, 7] and list(data) == [4, 1, 10, 11, 12, 9, 15]
    assert list(after.r) == [1, 0, 1, 3] and list(after.n) == [0, 0, 0, 0]
    streams, offsets, data, after = rings.drained(mask=[1, 1, 0, 1], min_len=2)
    assert list(streams) == [0] and list(offsets) == [0, 2] and list(data) == [4, 1]
    assert list(after.r) == [1, 0, 1, 2] and list(after.n) == [0, 0, 4, 1]
