"""The refusals of the filter and XModem host entry points (include/fskhip_next.h) that need no device, through ctypes on
libfskhip.so: every return code and the whole fskhip_last_error() string, in the order the checks are made, ending in the device
selection itself (no device here: the no-CPU-fallback text; with devices: an index one past the last).  Also the windowed-sinc
designs: their refusals and their taps for an odd and an even numTaps, bit for bit."""
import ctypes as C

import numpy as np
import pytest

F32, F64 = 0, 1
OK, E_INVALID, E_UNSUPPORTED, E_NO_DEVICE, E_OVERFLOW = 0, -1, -3, -4, -7


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def bad_device(L):
    """(device index, message) of a valid call that must end in the device selection's refusal"""
    n = L.fskhip_device_count()
    if n == 0:
        return 0, "no HIP device available (the engine has no CPU fallback)"
    return n, "device %d out of range (%d devices)" % (n, n)


def dbl(*v):
    return (C.c_double * max(1, len(v)))(*v)


def u32(*v):
    return (C.c_uint32 * len(v))(*v)   # (passed as it is: the call keeps it alive)


def test_fir_create_refusals_in_order(L):
    taps, h = dbl(0.5, 0.25), C.c_void_p()
    big = (C.c_double * 4097)()
    for args in ((0, None, 2, 1, F64, C.byref(h)), (0, taps, 2, 1, F64, None), (0, taps, 0, 1, F64, C.byref(h)), (0, taps, 2, 0, F64, C.byref(h)),
                 (0, None, 4097, 0, 7, None)):
        refused(L, L.fskhip_fir_create(*args), E_INVALID, "fskhip_fir_create: null/zero argument")
    refused(L, L.fskhip_fir_create(0, big, 4097, 1, 7, C.byref(h)), E_INVALID, "unknown precision 7")
    refused(L, L.fskhip_fir_create(0, taps, 2, 1, -1, C.byref(h)), E_INVALID, "unknown precision -1")
    refused(L, L.fskhip_fir_create(-5, big, 4097, 1, F32, C.byref(h)), E_UNSUPPORTED, "4097 taps do not fit the LDS tile (max 4096)")
    dev, text = bad_device(L)
    for prec in (F32, F64):
        refused(L, L.fskhip_fir_create(dev, taps, 2, 3, prec, C.byref(h)), E_NO_DEVICE, text)
    refused(L, L.fskhip_fir_create(dev, big, 4096, 1, F64, C.byref(h)), E_NO_DEVICE, text)
    assert h.value is None


def test_iir_create_refusals_in_order(L):
    b, a, zero, h = dbl(1.0, 0.5), dbl(1.0, -0.25), dbl(0.0, 1.0), C.c_void_p()
    long = dbl(*([1.0] * 11))
    create = L.fskhip_iir_create
    refused(L, create(0, None, 0, None, 0, 1, 7, None), E_INVALID, "fskhip_iir_create: null/zero argument")
    refused(L, create(0, b, 2, a, 2, 0, F64, C.byref(h)), E_INVALID, "fskhip_iir_create: null/zero argument")
    # the reference's three messages, before the precision, before the order, before the device
    refused(L, create(0, None, 2, None, 0, 1, 7, C.byref(h)), E_INVALID, "Feedforward coefficients (b) cannot be empty")
    refused(L, create(0, b, 0, a, 2, 1, F64, C.byref(h)), E_INVALID, "Feedforward coefficients (b) cannot be empty")
    refused(L, create(0, long, 11, None, 2, 1, 7, C.byref(h)), E_INVALID, "Feedback coefficients (a) cannot be empty")
    refused(L, create(0, b, 2, a, 0, 1, F64, C.byref(h)), E_INVALID, "Feedback coefficients (a) cannot be empty")
    refused(L, create(0, long, 11, zero, 2, 1, 7, C.byref(h)), E_INVALID, "First feedback coefficient (a[0]) cannot be zero")
    refused(L, create(0, long, 11, a, 2, 1, 7, C.byref(h)), E_INVALID, "unknown precision 7")
    refused(L, create(-5, long, 11, a, 2, 1, F64, C.byref(h)), E_UNSUPPORTED,
            "IIR order 10: the batched kernel keeps up to 8 past inputs and outputs in registers")
    refused(L, create(-5, b, 2, long, 10, 1, F32, C.byref(h)), E_UNSUPPORTED,
            "IIR order 9: the batched kernel keeps up to 8 past inputs and outputs in registers")
    dev, text = bad_device(L)
    for prec in (F32, F64):
        refused(L, create(dev, b, 2, a, 2, 3, prec, C.byref(h)), E_NO_DEVICE, text)
    refused(L, create(dev, long, 9, long, 9, 1, F64, C.byref(h)), E_NO_DEVICE, text)
    assert h.value is None


def test_device_index_refusals(L):
    """an index below zero or past the last device; with no device at all every index gets the no-device text"""
    n = L.fskhip_device_count()
    h, lens, crc = C.c_void_p(), u32(1), np.zeros(1, np.uint16)
    for dev in (-1, n, n + 7):
        text = "device %d out of range (%d devices)" % (dev, n) if n else "no HIP device available (the engine has no CPU fallback)"
        refused(L, L.fskhip_fir_create(dev, dbl(1.0), 1, 1, F64, C.byref(h)), E_NO_DEVICE, text)
        refused(L, L.fskhip_iir_create(dev, dbl(1.0), 1, dbl(1.0), 1, 1, F64, C.byref(h)), E_NO_DEVICE, text)
        refused(L, L.fskhip_crc16_host(dev, np.zeros(4, np.uint8).ctypes.data, 4, lens, 1, crc.ctypes.data), E_NO_DEVICE, text)


def test_crc16_host_refusals_in_order(L):
    data, crc = np.zeros((3, 8), np.uint8), np.zeros(3, np.uint16)
    lens = u32(8, 9, 100)
    call = L.fskhip_crc16_host
    assert call(-5, None, 0, None, 0, None) == OK                      # nothing to do: no pointer, no device
    refused(L, call(0, data.ctypes.data, 8, None, 3, crc.ctypes.data), E_INVALID, "fskhip_crc16_host: null buffer")
    refused(L, call(0, data.ctypes.data, 8, lens, 3, None), E_INVALID, "fskhip_crc16_host: null buffer")
    refused(L, call(0, data.ctypes.data, 8, lens, 3, crc.ctypes.data), E_INVALID, "lens[1] = 9 exceeds pitch 8")
    refused(L, call(0, None, 0, u32(0, 0, 1), 3, crc.ctypes.data), E_INVALID, "lens[2] = 1 exceeds pitch 0")
    dev, text = bad_device(L)
    refused(L, call(dev, data.ctypes.data, 8, u32(8, 0, 3), 3, crc.ctypes.data), E_NO_DEVICE, text)
    assert not crc.any()


def test_xmodem_serialize_host_refusals_in_order(L):
    pay, out, out_lens = np.zeros((2, 8), np.uint8), np.zeros((2, 13), np.uint8), np.zeros(2, np.uint32)
    P, O, OL = pay.ctypes.data, out.ctypes.data, out_lens.ctypes.data
    call = L.fskhip_xmodem_serialize_host
    assert call(-5, None, 0, None, None, 0, None, 0, None) == OK
    lens, seqs = u32(8, 8), u32(1, 2)
    for args in ((0, P, 8, None, seqs, 2, O, 13, OL), (0, P, 8, lens, None, 2, O, 13, OL),
                 (0, P, 8, lens, seqs, 2, None, 13, OL), (0, P, 8, lens, seqs, 2, O, 13, None)):
        refused(L, call(*args), E_INVALID, "fskhip_xmodem_serialize_host: null buffer")

    def rows(lens, seqs, payload_pitch=8, out_pitch=13, dev=0):
        return call(dev, P, payload_pitch, u32(*lens), u32(*seqs), 2, O, out_pitch, OL)

    # row by row, and within a row: sequence, length, payload pitch, slab
    refused(L, rows((7, 300), (1, 0)), E_INVALID, "Invalid sequence: 0. Must be 1-255.")
    refused(L, rows((300, 300), (256, 0)), E_INVALID, "Invalid sequence: 256. Must be 1-255.")
    refused(L, rows((7, 256), (1, 255)), E_INVALID, "Payload too large: 256. Max 255 bytes.")
    refused(L, rows((7, 9), (1, 255)), E_INVALID, "lens[1] = 9 exceeds payload_pitch 8")
    refused(L, rows((8, 3), (1, 0)), E_OVERFLOW, "row 0 needs 14 bytes, slab holds 13")
    refused(L, rows((7, 8), (1, 2), out_pitch=0), E_OVERFLOW, "row 0 needs 13 bytes, slab holds 0")
    dev, text = bad_device(L)
    refused(L, rows((7, 0), (1, 255), dev=dev), E_NO_DEVICE, text)
    assert not out.any() and not out_lens.any()


def test_xmodem_scan_host_refusals_in_order(L):
    by, data, res = np.zeros((2, 16), np.uint8), np.zeros((2, 16), np.uint8), np.zeros((2, 10), np.int32)
    B, D, R = by.ctypes.data, data.ctypes.data, res.ctypes.data
    call = L.fskhip_xmodem_scan_host
    assert call(-5, None, 0, None, None, 0, None, 0, None) == OK
    counts, exp = u32(16, 17), u32(1, 1)
    for args in ((0, B, 16, None, exp, 2, D, 16, R), (0, B, 16, counts, None, 2, D, 16, R),
                 (0, B, 16, counts, exp, 2, D, 16, None)):
        refused(L, call(*args), E_INVALID, "fskhip_xmodem_scan_host: null buffer")
    refused(L, call(0, B, 16, counts, exp, 2, D, 16, R), E_INVALID, "counts[1] = 17 exceeds pitch 16")
    refused(L, call(0, None, 0, u32(1, 0), exp, 2, None, 0, R), E_INVALID, "counts[0] = 1 exceeds pitch 0")
    dev, text = bad_device(L)
    refused(L, call(dev, B, 16, u32(16, 0), exp, 2, D, 16, R), E_NO_DEVICE, text)
    refused(L, call(dev, B, 16, u32(16, 0), exp, 2, None, 0, R), E_NO_DEVICE, text)
    assert not res.any()


def test_null_filter_handles(L):
    x = np.zeros(8, np.float64)
    X = x.ctypes.data
    for fn in (L.fskhip_fir_process_host, L.fskhip_iir_process_host, L.fskhip_iir_process_f64_host):
        refused(L, fn(None, X, 4, 4, X, 4), E_INVALID, "null filter")
        refused(L, fn(None, None, 0, 0, None, 0), E_INVALID, "null filter")       # before the n == 0 return
    for fn in (L.fskhip_fir_process_device, L.fskhip_iir_process_device, L.fskhip_iir_process_f64_device):
        refused(L, fn(None, X, 4, 4, X, 4, None), E_INVALID, "null filter")
        refused(L, fn(None, None, 0, 0, None, 0, None), E_INVALID, "null filter")
    for fn in (L.fskhip_fir_reset, L.fskhip_iir_reset):
        for stream in (-1, 0, 5):
            refused(L, fn(None, stream), E_INVALID, "null filter")
    assert L.fskhip_fir_destroy(None) == OK and L.fskhip_iir_destroy(None) == OK
    assert L.fskhip_fir_streams(None) == 0 and L.fskhip_iir_streams(None) == 0
    refused(L, L.fskhip_iir_get_coefficients(None, None, None, None, None), E_INVALID, "fskhip_iir_get_coefficients: null argument")


# the designs' taps as C99 hex floats: filters.ts:243-314 evaluated by this library (1000 Hz -- the band pass 1750 Hz, 800 Hz
# wide -- at 48 kHz); an even numTaps gives numTaps + 1 low-pass / high-pass taps, and numTaps band-pass taps
SINC_TAPS = {
    ("lowpass", 5): ['0x1.afeed1e702fd3p-9', '0x1.6f969096fd9c6p-6', '0x1.5555555555555p-5', '0x1.6f969096fd9c8p-6', '0x1.afeed1e702fd3p-9'],
    ("lowpass", 4): ['0x1.afeed1e702fd3p-9', '0x1.6f969096fd9c6p-6', '0x1.5555555555555p-5', '0x1.6f969096fd9c8p-6', '0x1.afeed1e702fd3p-9'],
    ("highpass", 5): ['-0x1.afeed1e702fd3p-9', '-0x1.6f969096fd9c6p-6', '0x1.eaaaaaaaaaaabp-1', '-0x1.6f969096fd9c8p-6', '-0x1.afeed1e702fd3p-9'],
    # (the reference negates numTaps = 4 of the five low-pass taps and adds 1 to none: filters.ts:274-286)
    ("highpass", 4): ['-0x1.afeed1e702fd3p-9', '-0x1.6f969096fd9c6p-6', '-0x1.5555555555555p-5', '-0x1.6f969096fd9c8p-6', '0x1.afeed1e702fd3p-9'],
    ("bandpass", 5): ['-0x1.f654f85632d6ep-16', '-0x1.b3dfba9ab5ecap-12', '0x1.2bceb3f22ba38p-8', '0x1.577fa442b1284p-5', '0x1.4e3b165cd8a83p-4'],
    ("bandpass", 4): ['-0x1.f654f85632d6ep-16', '-0x1.b3dfba9ab5ecap-12', '-0x1.22e9d0b0133c8p-9', '-0x1.7ca13bd828194p-8'],
}


def test_sinc_designs(L):
    buf = (C.c_double * 8)()
    for name in ("lowpass", "highpass"):
        fn = getattr(L, "fskhip_sinc_" + name)
        refused(L, fn(1000.0, 48000.0, 5, None), E_INVALID, "fskhip_sinc_%s: bad argument" % name)
        refused(L, fn(1000.0, 48000.0, 0, buf), E_INVALID, "fskhip_sinc_%s: bad argument" % name)
        for n_taps, n_out in ((5, 5), (4, 5)):
            for i in range(8):
                buf[i] = -7.0
            assert fn(1000.0, 48000.0, n_taps, buf) == n_out
            assert [float(v).hex() for v in buf[:n_out]] == SINC_TAPS[name, n_taps]
            assert list(buf[n_out:]) == [-7.0] * (8 - n_out)
    fn = L.fskhip_sinc_bandpass
    refused(L, fn(1750.0, 800.0, 48000.0, 5, None), E_INVALID, "fskhip_sinc_bandpass: bad argument")
    refused(L, fn(1750.0, 800.0, 48000.0, 0, buf), E_INVALID, "fskhip_sinc_bandpass: bad argument")
    for n_taps in (5, 4):
        for i in range(8):
            buf[i] = -7.0
        assert fn(1750.0, 800.0, 48000.0, n_taps, buf) == n_taps
        assert [float(v).hex() for v in buf[:n_taps]] == SINC_TAPS["bandpass", n_taps]
        assert list(buf[n_taps:]) == [-7.0] * (8 - n_taps)
