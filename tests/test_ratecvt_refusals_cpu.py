"""The rational rate converter without a GPU (include/fskhip_next.h: fskhip_ratecvt_*): the refusals of create, by code and whole text,
in the header's order, ending in the device selection itself; the null handle, which every other call refuses first (the refusals
behind it need a handle, so test_gpu_ratecvt.py holds them, in order); the symbols in the ctypes table; and what the Python classes
decide before they reach the library -- the ratio from the rates, the default design's length and its limit."""
import ctypes as C

import numpy as np
import pytest

import ratecvt_ref as rc
from test_next_refusals_cpu import E_INVALID, E_NO_DEVICE, E_UNSUPPORTED, F32, F64, OK, bad_device, dbl, refused

CAPTURE, PLAYBACK = 0, 1
SYMBOLS = ["create", "destroy", "streams", "history", "reset", "capture_device", "capture_host", "playback_device", "playback_host", "state_get", "state_set"]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def test_symbols_are_bound(L):
    from webaudio_modem_amd import _lib
    for name in SYMBOLS:
        assert "fskhip_ratecvt_" + name in _lib.SYMBOL_NAMES
        assert hasattr(L, "fskhip_ratecvt_" + name)
    assert (_lib.RATECVT_CAPTURE, _lib.RATECVT_PLAYBACK) == (CAPTURE, PLAYBACK)
    assert L.fskhip_abi_version() == 8


def test_create_refusals_in_order(L):
    taps, h = dbl(0.5, 0.25), C.c_void_p()
    big = (C.c_double * 4097)()
    create = L.fskhip_ratecvt_create
    # each refusal is met with everything behind it wrong as well
    for args in ((0, CAPTURE, 160, 147, None, 2, 1, F64, C.byref(h)), (0, CAPTURE, 160, 147, taps, 2, 1, F64, None), (0, 7, 0, 0, None, 0, 0, 7, None)):
        refused(L, create(*args), E_INVALID, "fskhip_ratecvt_create: null taps or out")
    for args in ((0, CAPTURE, 160, 147, taps, 0, 1, F64, C.byref(h)), (0, PLAYBACK, 147, 160, taps, 2, 0, F64, C.byref(h)), (0, 7, 0, 4, big, 0, 0, 7, C.byref(h))):
        refused(L, create(*args), E_INVALID, "fskhip_ratecvt_create: zero n_streams or n_taps")
    refused(L, create(0, 2, 0, 4, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: unknown direction 2")
    refused(L, create(0, -1, 160, 147, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: unknown direction -1")
    refused(L, create(0, CAPTURE, 0, 4, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: ratio 0 / 4 outside 1..256")
    refused(L, create(0, PLAYBACK, 257, 256, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: ratio 257 / 256 outside 1..256")
    refused(L, create(0, CAPTURE, 3, 0, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: ratio 3 / 0 outside 1..256")
    refused(L, create(0, PLAYBACK, 2, 300, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: ratio 2 / 300 outside 1..256")
    refused(L, create(0, CAPTURE, 6, 4, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: 6 / 4 is not in lowest terms")
    refused(L, create(0, PLAYBACK, 256, 256, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_ratecvt_create: 256 / 256 is not in lowest terms")
    refused(L, create(0, CAPTURE, 160, 147, big, 4097, 1, 7, C.byref(h)), E_INVALID, "unknown precision 7")
    refused(L, create(0, PLAYBACK, 1, 1, taps, 2, 1, -1, C.byref(h)), E_INVALID, "unknown precision -1")
    for direction in (CAPTURE, PLAYBACK):
        refused(L, create(-5, direction, 160, 147, big, 4097, 1, F32, C.byref(h)), E_UNSUPPORTED, "4097 taps do not fit the LDS tile (max 4096)")
    dev, text = bad_device(L)
    for direction, up, down, prec in ((CAPTURE, 160, 147, F32), (PLAYBACK, 147, 160, F64), (CAPTURE, 1, 1, F64), (PLAYBACK, 256, 255, F32), (CAPTURE, 1, 256, F32)):
        refused(L, create(dev, direction, up, down, taps, 2, 3, prec, C.byref(h)), E_NO_DEVICE, text)
    refused(L, create(dev, PLAYBACK, 147, 160, big, 4096, 1, F64, C.byref(h)), E_NO_DEVICE, text)
    assert h.value is None


def test_null_handles(L):
    x = np.zeros(8, np.float32)
    X = x.ctypes.data
    # the null handle comes before format, layout and the n_in == 0 return
    refused(L, L.fskhip_ratecvt_capture_device(None, X, 99, 99, 4, 0, None, 0, None), E_INVALID, "null rate converter")
    refused(L, L.fskhip_ratecvt_capture_host(None, None, 0, 0, 0, 0, None, 0), E_INVALID, "null rate converter")
    refused(L, L.fskhip_ratecvt_playback_device(None, X, 5, 0, None, X, 99, 99, 0, None), E_INVALID, "null rate converter")
    refused(L, L.fskhip_ratecvt_playback_host(None, None, 0, 0, None, None, 0, 0, 0), E_INVALID, "null rate converter")
    for stream in (-1, 0, 5):
        refused(L, L.fskhip_ratecvt_reset(None, stream), E_INVALID, "null rate converter")
    refused(L, L.fskhip_ratecvt_state_get(None, X), E_INVALID, "null rate converter")
    refused(L, L.fskhip_ratecvt_state_set(None, X), E_INVALID, "null rate converter")
    assert L.fskhip_ratecvt_destroy(None) == OK
    assert L.fskhip_ratecvt_streams(None) == 0 and L.fskhip_ratecvt_history(None) == 0


def test_python_classes_reduce_the_rates(L):
    import webaudio_modem_amd as wm
    for cls in (wm.CaptureConverter, wm.PlaybackConverter):
        assert cls.ratio(44100, 48000) == (160, 147) and cls.ratio(48000, 44100) == (147, 160)
        assert cls.ratio(8000, 48000) == (6, 1) and cls.ratio(48000, 8000) == (1, 6) and cls.ratio(48000, 48000) == (1, 1)
        assert cls.ratio(32000, 48000) == (3, 2) and cls.ratio(8000, 44100) == (441, 80) and cls.ratio(44100.0, 48000.0) == (160, 147)
        for bad in ((0, 48000), (44100.5, 48000), (48000, -1)):
            with pytest.raises(ValueError, match="rates must be positive whole numbers"):
                cls.ratio(*bad)
    assert rc.ratio(44100, 48000) == (160, 147) and rc.ratio(8000, 44100) == (441, 80)


def test_default_design(L):
    """16 max(L, M) + 1 taps at 0.45 of the lower rate, designed at L * in_rate, times L: 2 561 taps and 19 845 Hz both ways between
    44.1 and 48 kHz; a default past 4 096 taps is refused with the limit named, before any device call"""
    import webaudio_modem_amd as wm
    for cls, rates in ((wm.CaptureConverter, (44100, 48000)), (wm.PlaybackConverter, (48000, 44100)), (wm.CaptureConverter, (32000, 48000)),
                       (wm.PlaybackConverter, (48000, 8000))):
        taps = cls.default_taps(*rates)
        up, down = cls.ratio(*rates)
        assert len(taps) == 16 * max(up, down) + 1
        np.testing.assert_allclose(taps, rc.default_taps(*rates), rtol=0, atol=1e-13)
        assert abs(sum(taps) - up) < 0.01 * up
    assert len(wm.CaptureConverter.default_taps(44100, 48000)) == 2561 and 0.45 * 44100 == 19845.0
    for cls, rates in ((wm.CaptureConverter, (8000, 44100)), (wm.PlaybackConverter, (44100, 8000))):
        with pytest.raises(ValueError, match=r"needs 7057 taps, the limit is 4096"):
            cls.default_taps(*rates)
        with pytest.raises(ValueError, match=r"needs 7057 taps, the limit is 4096"):
            cls(rates[0], rates[1], 4)


def test_python_classes_fail_loudly_without_gpu(L):
    import webaudio_modem_amd as wm
    if L.fskhip_device_count() > 0:
        pytest.skip("a GPU is present")
    for cls, rates in ((wm.CaptureConverter, (44100, 48000)), (wm.PlaybackConverter, (48000, 44100))):
        with pytest.raises(wm.FskHipError) as ei:
            cls(rates[0], rates[1], 4)
        assert ei.value.code == E_NO_DEVICE and "no CPU fallback" in str(ei.value)
