"""The rate converter's calls of any length without a GPU (include/fskhip_next.h: "Rate conversion in calls of any length"):
  * the model (tests/ratecvt_any_ref.py): random cuts of a signal into calls of any length -- lengths 1 and calls that write
    nothing included -- give the uncut result, the same history and the same position, and the counts in integers are what the
    cuts add up to;
  * what the feature is for, through the model and the oracle: the default 44.1 <-> 48 kHz designs in cuts of 128 samples bring
    the default configuration back byte for byte, as tests/test_ratecvt_cpu.py does with whole periods;
  * the host arithmetic (csrc/fsk_ratecvt_plan.h: "Calls of any length") from a stand-alone program under AddressSanitizer and UBSan
    (tests/cpp/ratecvt_any_plan_check.cpp);
  * the library without a device: the new entry points are declared, exported and bound, they refuse a null handle first,
    fskhip_ratecvt_position(NULL) and the counts of a null handle are 0, and the ABI version stays 8.
The plan test and the library test fail without the feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ratecvt_any_ref as ra
import ratecvt_ref as rc
import samples_ref as sr
from conftest import ROOT
from oracle import pyoracle as po


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_counts_in_integers():
    assert ra.out_count_any(160, 147, 0, 128) == 140 and ra.out_count_any(160, 147, 128, 128) == 139 and ra.in_count_any(147, 160, 0, 128) == 139
    assert sum(ra.out_count_any(147, 160, pos, 1) == 0 for pos in range(160)) == 13
    for L, M in ((3, 2), (2, 3), (7, 5), (160, 147), (147, 160), (1, 4), (5, 1)):
        for pos in range(M):
            assert ra.out_count_any(L, M, pos, 0) == 0 and ra.in_count_any(L, M, pos, 0) == 0
            for n in (1, 2, M - 1, M, M + 1, 3 * M + 1):
                whole = ra.out_count_any(L, M, pos, n)
                assert whole == sum(1 for j in range((pos + n) * L // M + 2) if pos <= j * M // L < pos + n)
                if pos == 0 and n % M == 0:
                    assert whole == n // M * L
                for a in (0, 1, n // 2, n):
                    assert ra.out_count_any(L, M, pos, a) + ra.out_count_any(L, M, (pos + a) % M, n - a) == whole
                for n_out in range(1, whole + 2):
                    need = ra.in_count_any(L, M, pos, n_out)
                    assert ra.out_count_any(L, M, pos, need) >= n_out > ra.out_count_any(L, M, pos, need - 1)
                    assert L > M or ra.out_count_any(L, M, pos, need) == n_out


@pytest.mark.parametrize("L,M,n_taps", [(3, 2, 7), (2, 3, 8), (7, 5, 113), (160, 147, 2561), (147, 160, 2561), (1, 4, 9), (5, 1, 11)])
def test_model_is_cut_invariant_at_any_length(L, M, n_taps):
    rng = np.random.default_rng(L + 7 * M + n_taps)
    taps = rng.uniform(-1, 1, n_taps)
    N = 6 * M + M // 2 + 1
    x = rng.uniform(-1, 1, (3, N)).astype(np.float32)
    whole = ra.convert_whole(x, taps, L, M)
    H = rc.history(L, n_taps)
    hist = np.concatenate([np.zeros((3, H), np.float32), x], axis=1)[:, N:]
    assert whole.shape == (3, -(-N * L // M))
    # whole periods from position 0 are the existing model
    y, h, pos = ra.convert_any(x[:, :4 * M], taps, L, M)
    y0, h0 = rc.convert(x[:, :4 * M], taps, L, M)
    assert pos == 0 and np.array_equal(_bits(y), _bits(y0)) and np.array_equal(_bits(h), _bits(h0))
    zero_calls = 0
    for trial in range(4):
        if trial == 0:
            cuts = list(range(N + 1))                                     # all in ones
        else:
            cuts = [0] + sorted(set(rng.choice(np.arange(1, N), size=min(7, N - 1), replace=False).tolist())) + [N]
        h, pos, parts = None, 0, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            want = ra.out_count_any(L, M, pos, b - a)
            y, h, pos = ra.convert_any(x[:, a:b], taps, L, M, pos, h)
            assert y.shape == (3, want) and pos == b % M
            zero_calls += want == 0
            parts.append(y)
        assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole)) and np.array_equal(_bits(h), _bits(hist))
    assert zero_calls > 0 or L >= M                                        # (calls that write nothing were among them where they exist)


def test_round_trip_at_44100_in_cuts_of_128():
    """48 kHz modulate -> x 147 / 160 in calls of 128 -> s16 at 44.1 kHz -> x 160 / 147 in calls of 128 -> demodulate, default
    designs and configuration: all 32 bytes"""
    down_taps, up_taps = rc.default_taps(48000, 44100), rc.default_taps(44100, 48000)
    payload = bytes(range(40, 72))
    tx, rx = po.OracleCore(None), po.OracleCore(None)
    x = np.concatenate([np.zeros(480, np.float32), np.asarray(tx.modulate(payload), np.float32), np.zeros(4800, np.float32)])
    low, h, pos = [], None, 0
    for a in range(0, x.size, 128):
        y, h, pos = ra.playback_any(x[a:a + 128], down_taps, 147, 160, "s16", pos=pos, hist=h)
        low.append(y)
    low = np.concatenate(low, axis=1)
    assert low.shape == (1, -(-x.size * 147 // 160)) and low.dtype == sr.DTYPES["s16"]
    whole = rc.playback(np.concatenate([x, np.zeros(-x.size % 160, np.float32)]), down_taps, 147, 160, "s16")[0]
    assert np.array_equal(low, whole[:, :low.shape[1]])
    high, h, pos = [], None, 0
    for a in range(0, low.shape[1], 128):
        y, h, pos = ra.capture_any(low[:, a:a + 128], "s16", up_taps, 160, 147, pos, h)
        high.append(y)
    high = np.concatenate(high, axis=1)
    assert high.shape == (1, -(-low.shape[1] * 160 // 147))
    got, _eod = rx.demodulate(high[0])
    assert got == payload


def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ratecvt_any_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "ratecvt_any_plan_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


CONVERTER_CALLS = {"fskhip_ratecvt_capture_any_device": (None, 1, 0, 5, 5, None, 8, None, None),
                   "fskhip_ratecvt_playback_any_device": (None, 5, 5, None, None, 1, 0, 8, None, None),
                   "fskhip_ratecvt_capture_any_host": (None, 1, 0, 5, 5, None, 8, None),
                   "fskhip_ratecvt_playback_any_host": (None, 5, 5, None, None, 1, 0, 8, None)}
PROCESSOR_CALLS = {"fskhip_processor_process_ratecvt_any_device": (None,), "fskhip_processor_process_ratecvt_any_host": ()}
OTHERS = ("fskhip_ratecvt_position", "fskhip_ratecvt_position_set", "fskhip_ratecvt_out_count_any", "fskhip_ratecvt_in_count_any")


def test_library_without_a_device():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in list(CONVERTER_CALLS) + list(PROCESSOR_CALLS) + list(OTHERS):
        assert " %s(" % name in hdr and hasattr(raw, name) and name in _lib.SYMBOL_NAMES, name
    assert "Rate conversion in calls of any length (ABI 8, additions; FSKHIP_ABI_VERSION stays 8)" in hdr
    assert L.fskhip_abi_version() == 8
    # a null handle is refused before anything else is looked at: every other argument is wrong as well
    for name, args in CONVERTER_CALLS.items():
        assert getattr(L, name)(None, *args) == _lib.E_INVALID and L.fskhip_last_error().decode() == "null rate converter", name
    assert L.fskhip_ratecvt_position_set(None, 0) == _lib.E_INVALID and L.fskhip_last_error().decode() == "null rate converter"
    assert L.fskhip_ratecvt_position(None) == 0 and L.fskhip_ratecvt_out_count_any(None, 128) == 0 and L.fskhip_ratecvt_in_count_any(None, 128) == 0
    buf = np.zeros(64, np.uint8)
    for name, tail in PROCESSOR_CALLS.items():
        fn = getattr(L, name)
        assert fn(None, None, None, buf.ctypes.data + 1, 9, 9, 8, 0, buf.ctypes.data + 1, -1, 7, 8, 0, 0, *tail) == _lib.E_INVALID
        assert L.fskhip_last_error().decode() == "null processor"
        stand_in = np.full(4096, 5, np.uint32)       # (behind the null check nothing of the processor is read before a handle has been seen)
        assert fn(stand_in.ctypes.data, None, None, buf.ctypes.data, 4, 0, 8, 8, None, 0, 0, 0, 0, 0, *tail) == _lib.E_INVALID
        assert L.fskhip_last_error().decode() == "%s: unknown sample format 4" % name
        assert fn(stand_in.ctypes.data, None, None, buf.ctypes.data, 1, 0, 5, 5, None, 0, 0, 0, 0, 0, *tail) == _lib.E_INVALID
        assert L.fskhip_last_error().decode() == "%s: null capture handle" % name
        assert fn(stand_in.ctypes.data, None, None, None, 1, 0, 5, 5, buf.ctypes.data, 1, 0, 5, 5, 0, *tail) == _lib.E_INVALID
        assert L.fskhip_last_error().decode() == "%s: null playback handle" % name
        assert (stand_in == 5).all() and not buf.any()


def test_python_sends_converters_to_the_any_call_and_refuses_resamplers():
    from webaudio_modem_amd import CaptureConverter, Downsampler, PlaybackConverter, Upsampler
    from webaudio_modem_amd.processor import FSKProcessorBatch

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *args: self.calls.append((name, args)) or 0

    def handle(kind, n_streams, up, down):
        h = object.__new__(kind)
        h.n_streams, h.device, h.up, h.down = n_streams, 0, up, down
        h._h = id(h)
        return h

    b = object.__new__(FSKProcessorBatch)
    b.n_streams, b.flags, b.processDemodulationCallCount, b._h = 3, 0, 0, None
    b.engine = type("NoEngine", (), {"device": 0})()
    b._L = Recorder()
    cap, play = handle(CaptureConverter, 3, 160, 147), handle(PlaybackConverter, 3, 147, 160)
    out = b.process_samples_at_any(np.zeros((128, 3), np.uint8), upsampler=cap, n_out=129, downsampler=play)
    assert out.shape == (129, 3) and b.processDemodulationCallCount == 1
    b.process_samples_at_any_device(4096, "s16", "stream", 1, 4, cap, 8192, "f32", "stream", 127, 128, play, stream=7)
    assert [c[0] for c in b._L.calls] == ["fskhip_processor_process_ratecvt_any_host", "fskhip_processor_process_ratecvt_any_device"]
    assert b._L.calls[0][1][4:8] == (2, 1, 128, 3) and b._L.calls[0][1][9:] == (2, 1, 129, 3, 0)
    assert b._L.calls[1][1] == (None, cap._h, play._h, 4096, 1, 0, 1, 4, 8192, 0, 0, 127, 128, 0, 7)
    del b._L.calls[:]
    with pytest.raises(TypeError, match="upsampler is a Upsampler"):
        b.process_samples_at_any(np.zeros((128, 3), np.uint8), upsampler=handle(Upsampler, 3, 6, 1))
    with pytest.raises(TypeError, match="downsampler is a Downsampler"):
        b.process_samples_at_any(None, n_out=128, downsampler=handle(Downsampler, 3, 1, 6))
    with pytest.raises(TypeError, match="downsampler is a Downsampler"):
        b.process_samples_at_any_device(None, "s16", "stream", 0, 0, None, 8192, "f32", "stream", 8, 8, handle(Downsampler, 3, 1, 6))
    assert b._L.calls == [] and b.processDemodulationCallCount == 1
