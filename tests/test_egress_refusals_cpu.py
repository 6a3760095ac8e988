"""The refusals of fskhip_egress_device and fskhip_modulate_host_fmt (include/fskhip.h) that need no device, through ctypes on
libfskhip.so: every return code and the whole fskhip_last_error() string, in the order the checks are made."""
import numpy as np
import pytest

OK, E_INVALID, E_NOT_CONFIGURED = 0, -1, -2
F32, S16, MULAW, ALAW = 0, 1, 2, 3
STREAM, SAMPLE = 0, 1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, code, text):
    assert (rc, L.fskhip_last_error().decode()) == (code, text)


def test_egress_device_refusals_in_order(L):
    src, lens, dst = np.zeros(64, np.float32), np.zeros(16, np.uint32), np.full(64, 0x5A, np.uint8)
    SRC, LENS, DST = src.ctypes.data, lens.ctypes.data, dst.ctypes.data
    eg = L.fskhip_egress_device
    # format, then layout, before anything else is looked at
    refused(L, eg(None, 0, None, 2, 8, 7, 9, None, 0, None), E_INVALID, "fskhip_egress_device: unknown sample format 7")
    refused(L, eg(None, 0, None, 2, 8, -1, STREAM, None, 0, None), E_INVALID, "fskhip_egress_device: unknown sample format -1")
    refused(L, eg(None, 0, None, 2, 8, S16, 2, None, 0, None), E_INVALID, "fskhip_egress_device: unknown layout 2")
    refused(L, eg(None, 0, None, 2, 8, ALAW, -1, None, 0, None), E_INVALID, "fskhip_egress_device: unknown layout -1")
    # nothing to do is no error and needs no pointers, whatever else is passed
    assert eg(None, 0, None, 0, 8, S16, STREAM, None, 0, None) == OK
    assert eg(None, 0, None, 5, 0, ALAW, SAMPLE, None, 0, None) == OK
    assert eg(SRC + 1, 0, LENS + 1, 0, 0, F32, STREAM, DST + 1, 0, None) == OK
    # null buffers (d_lens may be null), pitches, alignments
    refused(L, eg(None, 8, LENS, 2, 8, S16, STREAM, DST, 8, None), E_INVALID, "fskhip_egress_device: null buffer")
    refused(L, eg(SRC, 8, LENS, 2, 8, S16, STREAM, None, 8, None), E_INVALID, "fskhip_egress_device: null buffer")
    for lay in (STREAM, SAMPLE):
        refused(L, eg(SRC, 7, None, 2, 8, S16, lay, DST, 8, None), E_INVALID, "fskhip_egress_device: src_pitch 7 < n_per_stream 8")
    refused(L, eg(SRC, 8, None, 2, 8, S16, STREAM, DST, 7, None), E_INVALID, "fskhip_egress_device: dst_pitch 7 < n_per_stream 8")
    refused(L, eg(SRC, 4, None, 9, 4, MULAW, SAMPLE, DST, 8, None), E_INVALID, "fskhip_egress_device: frame pitch 8 < n_streams 9")
    text = "fskhip_egress_device: a buffer is not aligned to its element size"
    for off in (1, 2, 3):
        refused(L, eg(SRC + off, 8, None, 2, 8, MULAW, STREAM, DST, 8, None), E_INVALID, text)
        refused(L, eg(SRC, 8, LENS + off, 2, 8, MULAW, STREAM, DST, 8, None), E_INVALID, text)
        refused(L, eg(SRC, 8, None, 2, 8, F32, STREAM, DST + off, 8, None), E_INVALID, text)
    refused(L, eg(SRC, 8, None, 2, 8, S16, SAMPLE, DST + 1, 8, None), E_INVALID, text)
    assert (dst == 0x5A).all()
    # a valid call ends at the device: launched where there is one (tests/test_gpu_egress.py), refused loudly where there is none
    if L.fskhip_device_count() == 0:
        for fmt, off in ((S16, 2), (MULAW, 1), (ALAW, 3), (F32, 4)):
            refused(L, eg(SRC, 8, LENS, 2, 8, fmt, SAMPLE, DST + off, 2, None), -4, "no HIP device available (the engine has no CPU fallback)")
        assert (dst == 0x5A).all()


def test_modulate_host_fmt_refusals_without_an_engine(L):
    pay, lens, out, out_lens = np.zeros(8, np.uint8), np.zeros(1, np.uint32), np.zeros(64, np.int16), np.zeros(1, np.uint32)
    mod = lambda fmt, lay: L.fskhip_modulate_host_fmt(None, pay.ctypes.data, lens.ctypes.data, 8, fmt, lay, out.ctypes.data, 64, 64,   # noqa: E731
                                                      out_lens.ctypes.data)
    # format and layout are checked before the engine is looked at, as fskhip_demodulate_host_fmt does
    refused(L, mod(4, STREAM), E_INVALID, "fskhip_modulate_host_fmt: unknown sample format 4")
    refused(L, mod(S16, 2), E_INVALID, "fskhip_modulate_host_fmt: unknown layout 2")
    for fmt in (F32, S16, MULAW, ALAW):
        for lay in (STREAM, SAMPLE):
            refused(L, mod(fmt, lay), E_NOT_CONFIGURED, "FSK modulator not configured")
    refused(L, L.fskhip_modulate_host_fmt(None, None, None, 0, S16, STREAM, None, 0, 0, None), E_NOT_CONFIGURED, "FSK modulator not configured")
    # the float call's own refusal, for comparison: the same code and text
    refused(L, L.fskhip_modulate_host(None, pay.ctypes.data, lens.ctypes.data, 8, out.ctypes.data, 16, out_lens.ctypes.data), E_NOT_CONFIGURED,
            "FSK modulator not configured")
    refused(L, L.fskhip_modulate_device(None, pay.ctypes.data, lens.ctypes.data, 8, out.ctypes.data, 16, out_lens.ctypes.data, None), E_NOT_CONFIGURED,
            "FSK modulator not configured")
    assert not out.any() and not out_lens.any()
