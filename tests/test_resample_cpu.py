"""The resampler without a GPU (include/fskhip_next.h: fskhip_resampler_*):
  * the refusals of create and of the process calls that need no device, by code and whole text, in the header's order, ending in the
    device selection itself;
  * the model (tests/resample_ref.py) against np.convolve -- the model's own sanity bar, not the kernels';
  * what the feature is for, through the model: modulate at 48 kHz, decimate by 6 with the default design, a trunk format at 8 kHz,
    interpolate by 6, demodulate -- every payload byte comes back for the default configuration, Bell 202 and 300 baud through s16,
    mu-law and A-law;
  * the host arithmetic (csrc/fsk_resample_plan.h) from a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as rr
import samples_ref as sr
from conftest import ROOT
from oracle import pyoracle as po
from test_next_refusals_cpu import E_INVALID, E_NO_DEVICE, E_UNSUPPORTED, F32, F64, OK, bad_device, dbl, refused

UP, DOWN = 0, 1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def test_create_refusals_in_order(L):
    taps, h = dbl(0.5, 0.25), C.c_void_p()
    big = (C.c_double * 4097)()
    create = L.fskhip_resampler_create
    for args in ((0, UP, 6, None, 2, 1, F64, C.byref(h)), (0, UP, 6, taps, 2, 1, F64, None), (0, 7, 99, None, 0, 0, 7, None)):
        refused(L, create(*args), E_INVALID, "fskhip_resampler_create: null taps or out")
    for args in ((0, UP, 6, taps, 0, 1, F64, C.byref(h)), (0, DOWN, 6, taps, 2, 0, F64, C.byref(h)), (0, 7, 99, big, 0, 0, 7, C.byref(h))):
        refused(L, create(*args), E_INVALID, "fskhip_resampler_create: zero n_streams or n_taps")
    refused(L, create(0, 2, 99, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_resampler_create: unknown direction 2")
    refused(L, create(0, -1, 6, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_resampler_create: unknown direction -1")
    refused(L, create(0, UP, 0, big, 4097, 1, 7, C.byref(h)), E_INVALID, "fskhip_resampler_create: factor 0 outside 1..32")
    refused(L, create(0, DOWN, 33, taps, 2, 1, F64, C.byref(h)), E_INVALID, "fskhip_resampler_create: factor 33 outside 1..32")
    refused(L, create(0, UP, 32, big, 4097, 1, 7, C.byref(h)), E_INVALID, "unknown precision 7")
    refused(L, create(0, DOWN, 1, taps, 2, 1, -1, C.byref(h)), E_INVALID, "unknown precision -1")
    for direction in (UP, DOWN):
        refused(L, create(-5, direction, 6, big, 4097, 1, F32, C.byref(h)), E_UNSUPPORTED, "4097 taps do not fit the LDS tile (max 4096)")
    dev, text = bad_device(L)
    for direction, factor, prec in ((UP, 1, F32), (DOWN, 32, F64), (UP, 6, F64)):
        refused(L, create(dev, direction, factor, taps, 2, 3, prec, C.byref(h)), E_NO_DEVICE, text)
    refused(L, create(dev, DOWN, 6, big, 4096, 1, F64, C.byref(h)), E_NO_DEVICE, text)
    assert h.value is None


def test_null_handles(L):
    x = np.zeros(8, np.float32)
    X = x.ctypes.data
    refused(L, L.fskhip_resampler_up_device(None, X, 99, 99, 4, 0, None, 0, None), E_INVALID, "null resampler")
    refused(L, L.fskhip_resampler_up_host(None, None, 0, 0, 0, 0, None, 0), E_INVALID, "null resampler")      # before the n_in == 0 return
    refused(L, L.fskhip_resampler_down_device(None, X, 5, 0, None, X, 99, 99, 0, None), E_INVALID, "null resampler")
    refused(L, L.fskhip_resampler_down_host(None, None, 0, 0, None, None, 0, 0, 0), E_INVALID, "null resampler")
    for stream in (-1, 0, 5):
        refused(L, L.fskhip_resampler_reset(None, stream), E_INVALID, "null resampler")
    refused(L, L.fskhip_resampler_state_get(None, X), E_INVALID, "null resampler")
    refused(L, L.fskhip_resampler_state_set(None, X), E_INVALID, "null resampler")
    assert L.fskhip_resampler_destroy(None) == OK
    assert L.fskhip_resampler_streams(None) == 0 and L.fskhip_resampler_history(None) == 0


def test_python_classes_fail_loudly_without_gpu(L):
    import webaudio_modem_amd as wm
    if L.fskhip_device_count() > 0:
        pytest.skip("a GPU is present")
    for cls in (wm.Upsampler, wm.Downsampler):
        with pytest.raises(wm.FskHipError) as ei:
            cls(6, 4)
        assert ei.value.code == E_NO_DEVICE and "no CPU fallback" in str(ei.value)
        with pytest.raises(ValueError, match="factor 33 outside 1..32"):
            cls(33, 4)


def test_default_design_is_the_models(L):
    """16 L + 1 taps at 0.45 of the low rate; 97 taps and 3 600 Hz for 8 kHz <-> 48 kHz; the up direction carries the gain L"""
    from webaudio_modem_amd import FilterDesign
    for factor, rate in ((6, 8000), (2, 8000), (3, 16000)):
        taps = FilterDesign.sincLowpass(0.45 * rate, factor * rate, 16 * factor + 1)
        assert len(taps) == 16 * factor + 1
        np.testing.assert_allclose(taps, rr.default_taps(factor, rate), rtol=0, atol=1e-16)
    assert abs(rr.default_taps(6).sum() - 1.0) < 0.01 and abs(rr.default_taps(6, up=True).sum() - 6.0) < 0.06


@pytest.mark.parametrize("factor,n_taps", [(1, 5), (2, 1), (3, 13), (6, 97), (6, 5)])
def test_model_against_convolve(factor, n_taps):
    rng = np.random.default_rng(factor * 100 + n_taps)
    taps = rng.uniform(-1, 1, n_taps)
    bar = 1e-6 * np.abs(taps).sum()
    x = rng.integers(-32768, 32768, (3, 50)).astype(np.int16)
    z = np.zeros((3, 50 * factor))
    z[:, ::factor] = x / 32768.0
    want = np.stack([np.convolve(r, taps)[:r.size] for r in z])
    got = rr.up(x, "s16", taps, factor)
    assert got.dtype == np.float32 and got.shape == want.shape and np.abs(got - want).max() <= bar
    u = rng.uniform(-1, 1, (3, 20 * factor)).astype(np.float32)
    want = np.stack([np.convolve(r.astype(np.float64), taps)[:r.size] for r in u])[:, ::factor]
    got = rr.down(u, taps, factor, "f32")
    assert got.shape == want.shape and np.abs(got - want).max() <= bar
    # the delay lines carry: two calls are one
    f = [po.FIR(list(taps)) for _ in range(3)]
    cut = 7 * factor
    two = np.concatenate([rr.down(u[:, :cut], taps, factor, "s16", filters=f), rr.down(u[:, cut:], taps, factor, "s16", filters=f)], axis=1)
    assert np.array_equal(two, rr.down(u, taps, factor, "s16"))
    # lens: the row reads as zeros from there on, and the tail ends in silence
    lens = [0, 5, 20 * factor]
    got = rr.down(u, taps, factor, "mulaw", lens=lens)
    assert (got[0] == sr.silence("mulaw")).all() and (got[1, (5 + n_taps - 1 + factor - 1) // factor:] == sr.silence("mulaw")).all()
    assert np.array_equal(got[2], rr.down(u, taps, factor, "mulaw")[2])


CONFIGS = {"default": None, "bell202": dict(baudRate=1200, markFrequency=1200, spaceFrequency=2200),
           "300baud": dict(baudRate=300, markFrequency=1650, spaceFrequency=1850)}


@pytest.mark.parametrize("fmt", ["s16", "mulaw", "alaw"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_round_trip_at_8_khz_through_the_model(cfg, fmt):
    """48 kHz modulate -> / 6 -> trunk format at 8 kHz -> x 6 -> demodulate, default designs (97 taps, 3 600 Hz): all 32 bytes"""
    payload = bytes(range(40, 72))
    tx, rx = po.OracleCore(CONFIGS[cfg]), po.OracleCore(CONFIGS[cfg])
    x = np.concatenate([np.zeros(480, np.float32), np.asarray(tx.modulate(payload), np.float32), np.zeros(4800, np.float32)])
    x = x[:x.size // 6 * 6]
    low = rr.down(x, rr.default_taps(6), 6, fmt)
    assert low.shape == (1, x.size // 6) and low.dtype == sr.DTYPES[fmt]
    high = rr.up(low, fmt, rr.default_taps(6, up=True), 6)
    got, _eod = rx.demodulate(high[0])
    assert got == payload


def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resample_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "resample_plan_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
