"""Capture formats without a GPU (include/fskhip.h: fskhip_sample_bytes, fskhip_ingest_device, fskhip_demodulate_host_fmt): the element
sizes, the numpy decode reference the GPU tests use (tests/samples_ref.py) against Python's audioop for every code, the argument
checks that need no device, and -- with no device -- the loud failure of the two compute entry points."""
import ctypes as C

import numpy as np
import pytest

import samples_ref as ir


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib


def test_sample_bytes(lib):
    L = lib.lib()
    assert [L.fskhip_sample_bytes(f) for f in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_MULAW, lib.SAMPLES_ALAW)] == [4, 2, 1, 1]
    assert [L.fskhip_sample_bytes(f) for f in (4, -1, 1000)] == [0, 0, 0]
    assert (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_MULAW, lib.SAMPLES_ALAW) == (0, 1, 2, 3)
    assert (lib.LAYOUT_STREAM_MAJOR, lib.LAYOUT_SAMPLE_MAJOR) == (0, 1)


def test_decode_reference_is_audioop_for_every_code():
    audioop = pytest.importorskip("audioop")
    codes = np.arange(256, dtype=np.uint8)
    for fmt, fn, top in (("mulaw", audioop.ulaw2lin, 32124), ("alaw", audioop.alaw2lin, 32256)):
        want = np.frombuffer(fn(codes.tobytes(), 2), dtype="<i2").astype(np.int32)
        got = ir.mulaw_to_linear(codes) if fmt == "mulaw" else ir.alaw_to_linear(codes)
        assert np.array_equal(got, want), fmt
        assert got.max() == top and got.min() == -top
    # 16-bit PCM: audioop's own widening of every int16 value to 32 bits is the value times 2^16
    s16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    wide = np.frombuffer(audioop.lin2lin(s16.astype("<i2").tobytes(), 2, 4), dtype="<i4")
    assert np.array_equal(ir.decode(s16, "s16", np.float64) * 32768.0 * 65536.0, wide.astype(np.float64))


def test_every_decoded_value_is_exact_in_float32():
    codes = np.arange(256, dtype=np.uint8)
    s16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    for fmt, x in (("mulaw", codes), ("alaw", codes), ("s16", s16)):
        f32, f64 = ir.decode(x, fmt, np.float32), ir.decode(x, fmt, np.float64)
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), f64), fmt
        assert np.array_equal(f64 * 32768.0, np.rint(f64 * 32768.0)) and np.abs(f64).max() <= 1.0
    # quantise() picks the nearest table entry: every table value is its own image
    for fmt in ("mulaw", "alaw"):
        t = ir.decode(codes, fmt)
        assert np.array_equal(ir.decode(ir.quantise(t, fmt), fmt), t)
    assert np.array_equal(ir.quantise(ir.decode(s16, "s16"), "s16"), s16)


def test_argument_checks_need_no_device(lib):
    L = lib.lib()
    src, dst = np.zeros(64, np.int16), np.zeros(64, np.float32)
    ing = lambda *a: L.fskhip_ingest_device(*a)   # noqa: E731
    err = lambda: L.fskhip_last_error().decode()  # noqa: E731
    assert ing(src.ctypes.data, 7, 0, 2, 8, 8, dst.ctypes.data, 8, None) == lib.E_INVALID and "format 7" in err()
    assert ing(src.ctypes.data, 1, 2, 2, 8, 8, dst.ctypes.data, 8, None) == lib.E_INVALID and "layout 2" in err()
    assert ing(None, 1, 0, 2, 8, 8, dst.ctypes.data, 8, None) == lib.E_INVALID and "null" in err()
    assert ing(src.ctypes.data, 1, 0, 2, 8, 8, None, 8, None) == lib.E_INVALID
    assert ing(src.ctypes.data, 1, 0, 2, 8, 7, dst.ctypes.data, 8, None) == lib.E_INVALID and "src_pitch 7" in err()
    assert ing(src.ctypes.data, 1, 0, 2, 8, 8, dst.ctypes.data, 7, None) == lib.E_INVALID and "dst_pitch 7" in err()
    assert ing(src.ctypes.data, 1, 1, 9, 4, 8, dst.ctypes.data, 4, None) == lib.E_INVALID and "frame pitch 8" in err()
    assert ing(src.ctypes.data + 1, 1, 0, 2, 8, 8, dst.ctypes.data, 8, None) == lib.E_INVALID and "aligned" in err()
    assert ing(src.ctypes.data, 1, 0, 2, 8, 8, dst.ctypes.data + 2, 8, None) == lib.E_INVALID
    # nothing to do is no error and needs no pointers, whatever else is passed
    assert ing(None, 1, 0, 0, 8, 8, None, 8, None) == lib.OK
    assert ing(None, 3, 1, 5, 0, 5, None, 0, None) == lib.OK
    # the host call checks format and layout before it looks at the engine
    dem = lambda fmt, lay: L.fskhip_demodulate_host_fmt(None, src.ctypes.data, fmt, lay, 8, 8, None, 0, None, None, 0)  # noqa: E731
    assert dem(4, 0) == lib.E_INVALID and "format 4" in err()
    assert dem(1, -1) == lib.E_INVALID and "layout -1" in err()
    assert dem(1, 1) == lib.E_NOT_CONFIGURED


def test_python_argument_checks():
    from webaudio_modem_amd.engine import sample_args
    with pytest.raises(ValueError, match="mulaw"):
        sample_args(np.zeros((2, 8), np.uint8))
    with pytest.raises(ValueError, match="dtype"):
        sample_args(np.zeros((2, 8), np.float64))
    with pytest.raises(ValueError, match="format"):
        sample_args(np.zeros((2, 8), np.int16), fmt="pcm24")
    with pytest.raises(ValueError, match="int16"):
        sample_args(np.zeros((2, 8), np.uint8), fmt="s16")
    with pytest.raises(ValueError, match="layout"):
        sample_args(np.zeros((2, 8), np.int16), layout="planar")
    a = np.zeros((10, 7), np.int16)
    assert sample_args(a)[1:] == (1, 0, 10, 7, 7)
    assert sample_args(a, layout="sample")[1:] == (1, 1, 7, 10, 7)
    x, *rest = sample_args(a[:, 2:5], layout="sample")           # a shard's column block: no copy, the full frame pitch
    assert rest == [1, 1, 3, 10, 7] and x.ctypes.data == a.ctypes.data + 4
    x, *rest = sample_args(a[3:6], fmt="s16")                    # ... and its row block
    assert rest == [1, 0, 3, 7, 7] and x.ctypes.data == a[3:].ctypes.data
    x, *rest = sample_args(a.T)                                  # anything else is copied
    assert rest == [1, 0, 7, 10, 10] and x.flags.c_contiguous
    assert sample_args(np.zeros((4, 6), np.uint8), fmt="alaw")[1] == 3


def test_compute_entry_points_fail_loudly_without_gpu(lib):
    import webaudio_modem_amd as wm
    L = lib.lib()
    if L.fskhip_device_count() > 0:
        pytest.skip("a GPU is present")
    src, dst = np.zeros(64, np.int16), np.zeros(64, np.float32)
    with pytest.raises(wm.FskHipError) as ei:
        wm.ingest_device(src.ctypes.data, "s16", "stream", 2, 8, 8, dst.ctypes.data, 8)
    assert ei.value.code == lib.E_NO_DEVICE and "no CPU fallback" in str(ei.value)
    # no engine can exist: the host call has nothing to run on, and says so
    out, counts = np.zeros(8, np.uint8), np.zeros(1, np.uint32)
    rc = L.fskhip_demodulate_host_fmt(None, src.ctypes.data, 1, 0, 8, 8, out.ctypes.data, 8, counts.ctypes.data, None, 0)
    assert rc == lib.E_NOT_CONFIGURED and "not configured" in L.fskhip_last_error().decode()
    with pytest.raises(wm.FskHipError) as ei:
        wm.FSKEngine(1, {}).demodulate_samples(src.reshape(1, -1))
    assert ei.value.code == lib.E_NO_DEVICE
