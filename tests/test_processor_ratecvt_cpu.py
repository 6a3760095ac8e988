"""fskhip_processor_process_ratecvt_host / _device (include/fskhip_next.h) without a GPU:
  * the symbols are declared in the header, exported and bound, and the ABI version stays 8;
  * what they refuse first, through ctypes on libfskhip.so -- every return code and the whole fskhip_last_error() string, in the
    header's order: a null processor, an unknown format or layout (input side first), then a side that has a buffer and no handle.
    Behind the null check these read nothing of the processor, so a stand-in block of memory serves as one
    (tests/test_gpu_processor_ratecvt.py goes on from there with live handles);
  * the Python argument checks of FSKProcessorBatch.process_samples_at with converters, on a batch without a device whose library
    is a recorder: converters are accepted up to the library call, the call that is made and its arguments; one call may not mix
    a resampler and a converter; the two counts are whole periods; stream count and device;
  * how the call chooses between its fused TX kernel and the two launches it replaces (csrc/fsk_processor_rate_plan.h:
    processor_ratecvt_plan), from a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OK, E_INVALID = 0, -1
F32, S16, MULAW, ALAW = 0, 1, 2, 3
STREAM, SAMPLE = 0, 1
S = 5
FORMS = (("fskhip_processor_process_ratecvt_host", ()), ("fskhip_processor_process_ratecvt_device", (None,)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, text):
    assert (rc, L.fskhip_last_error().decode()) == (E_INVALID, text)


def test_symbols_are_declared_exported_and_bound(L):
    from webaudio_modem_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    launch = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_launch.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, _tail in FORMS:
        assert "int %s(fskhip_processor *p, fskhip_ratecvt *capture, fskhip_ratecvt *playback, const void *" % name in hdr
        assert hasattr(raw, name) and name in _lib.SYMBOL_NAMES
    # each launcher the call goes through is declared once, where its callers and its definition both see it
    assert launch.count("hipError_t launch_processor_io_ratecvt(") == 1 and launch.count("hipError_t launch_ratecvt(") == 1
    assert L.fskhip_abi_version() == 8


@pytest.mark.parametrize("name,tail", FORMS)
def test_first_refusals_in_order(L, name, tail):
    fn = getattr(L, name)
    stand_in = np.full(4096, S, np.uint32)          # (never read before a handle has been seen; see the module's text)
    P = stand_in.ctypes.data
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data

    def call(p, cap, play, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch):
        return fn(p, cap, play, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch, 0, *tail)

    # 1. a null processor, before anything else is looked at
    refused(L, call(None, None, None, None, MULAW, SAMPLE, 0, 0, None, MULAW, SAMPLE, 0, 0), "null processor")
    refused(L, call(None, None, None, B + 1, 9, 9, 8, 0, B + 1, -1, 7, 8, 0), "null processor")
    # 2. an unknown format, then layout: the input side first, a NULL side included, before any handle is asked for
    refused(L, call(P, None, None, B + 1, 4, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown sample format 4" % name)
    refused(L, call(P, None, None, None, -1, STREAM, 0, 0, None, F32, STREAM, 0, 0), "%s: unknown sample format -1" % name)
    refused(L, call(P, None, None, B + 1, S16, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown layout 2" % name)
    refused(L, call(P, None, None, B + 1, S16, SAMPLE, 8, 0, B + 1, 5, 7, 8, 0), "%s: unknown sample format 5" % name)
    refused(L, call(P, None, None, B + 1, S16, SAMPLE, 8, 0, B + 1, ALAW, -1, 8, 0), "%s: unknown layout -1" % name)
    # 3. a side that has a buffer needs its handle: the input side first, before pitches, alignments and the multiples
    refused(L, call(P, None, None, B + 1, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "%s: null capture handle" % name)
    refused(L, call(P, None, None, None, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "%s: null playback handle" % name)
    assert (stand_in == S).all() and not buf.any()


class _Recorder:
    """a library whose every entry point records its call and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or OK


class _NoDevice:
    """FSKProcessorBatch.process_samples_at's argument checks need the stream count only: a batch without a processor behind it,
    over a library that records what it is asked"""

    def __new__(cls, n_streams):
        from webaudio_modem_amd.processor import FSKProcessorBatch
        b = object.__new__(FSKProcessorBatch)
        b.n_streams, b.flags, b.processDemodulationCallCount, b._h = n_streams, 0, 0, None
        b.engine = type("NoEngine", (), {"device": 0})()
        b._L = _Recorder()
        return b


def _handle(kind, n_streams, device=0, up=1, down=1):
    """a resampler or converter as the checks see one, without a device (_h: a number to know it by)"""
    h = object.__new__(kind)
    h.n_streams, h.device, h.up, h.down = n_streams, device, up, down
    h._h = id(h)
    return h


def test_python_accepts_converters_up_to_the_library_call():
    from webaudio_modem_amd import CaptureConverter, Downsampler, PlaybackConverter, Upsampler
    b = _NoDevice(3)
    cap, play = _handle(CaptureConverter, 3, up=160, down=147), _handle(PlaybackConverter, 3, up=147, down=160)
    frames = np.zeros((294, 3), np.uint8)
    out = b.process_samples_at(frames, upsampler=cap, n_out=441, downsampler=play)
    assert out.shape == (441, 3) and out.dtype == np.uint8 and b.processDemodulationCallCount == 1
    (name, args), = b._L.calls
    assert name == "fskhip_processor_process_ratecvt_host"
    assert args[:3] == (None, cap._h, play._h) and args[4:8] == (MULAW, SAMPLE, 294, 3) and args[9:] == (MULAW, SAMPLE, 441, 3, 0)
    # either side alone, the other side's handle not looked at; zero lengths are whole periods
    del b._L.calls[:]
    assert b.process_samples_at(np.zeros((3, 147), np.int16), "s16", "stream", cap) is None
    assert b.process_samples_at(None, n_out=147, out_fmt="alaw", out_layout="stream", downsampler=play).shape == (3, 147)
    assert b.process_samples_at(np.zeros((0, 3), np.uint8), upsampler=cap) is None
    b.process_samples_at_device(4096, "s16", "stream", 147, 160, cap, 8192, "f32", "stream", 294, 296, play, stream=7)
    b.process_samples_at_device(None, "s16", "stream", 0, 0, None, 8192, "f32", "stream", 294, 296, play)
    assert [c[0] for c in b._L.calls] == ["fskhip_processor_process_ratecvt_host"] * 3 + ["fskhip_processor_process_ratecvt_device"] * 2
    assert b._L.calls[3][1] == (None, cap._h, play._h, 4096, S16, STREAM, 147, 160, 8192, F32, STREAM, 294, 296, 0, 7)
    assert b._L.calls[4][1][:4] == (None, None, play._h, None)
    # resamplers still go where they went
    del b._L.calls[:]
    b.process_samples_at(frames, upsampler=_handle(Upsampler, 3), n_out=8, downsampler=_handle(Downsampler, 3))
    b.process_samples_at_device(None, "mulaw", "sample", 0, 3, None, 4096, "mulaw", "sample", 8, 3, _handle(Downsampler, 3))
    assert [c[0] for c in b._L.calls] == ["fskhip_processor_process_rate_host", "fskhip_processor_process_rate_device"]


def test_python_argument_checks_with_converters():
    from webaudio_modem_amd import CaptureConverter, Downsampler, PlaybackConverter, Upsampler
    b = _NoDevice(3)
    cap, play = _handle(CaptureConverter, 3, up=160, down=147), _handle(PlaybackConverter, 3, up=147, down=160)
    up, down = _handle(Upsampler, 3), _handle(Downsampler, 3)
    frames = np.zeros((294, 3), np.uint8)
    # a converter of the other direction is as wrong as a resampler of the other direction, in the existing words
    with pytest.raises(ValueError, match="upsampler must be a filters.Upsampler, got PlaybackConverter"):
        b.process_samples_at(frames, upsampler=play)
    with pytest.raises(ValueError, match="downsampler must be a filters.Downsampler, got CaptureConverter"):
        b.process_samples_at(None, n_out=147, downsampler=cap)
    with pytest.raises(ValueError, match="upsampler must be a filters.Upsampler, got NoneType"):
        b.process_samples_at(frames, n_out=147, downsampler=play)
    # one call, one kind: the message names both types
    with pytest.raises(ValueError, match="CaptureConverter.*Downsampler"):
        b.process_samples_at(frames, upsampler=cap, n_out=8, downsampler=down)
    with pytest.raises(ValueError, match="Upsampler.*PlaybackConverter"):
        b.process_samples_at(frames, upsampler=up, n_out=147, downsampler=play)
    with pytest.raises(ValueError, match="CaptureConverter.*Downsampler"):
        b.process_samples_at_device(4096, "s16", "stream", 147, 160, cap, 8192, "f32", "stream", 8, 8, down)
    # whole periods
    with pytest.raises(ValueError, match="293 samples per stream are not a multiple of the converter's down factor 147"):
        b.process_samples_at(frames[:293], upsampler=cap)
    with pytest.raises(ValueError, match="n_out 440 is not a multiple of the converter's up factor 147"):
        b.process_samples_at(frames, upsampler=cap, n_out=440, downsampler=play)
    with pytest.raises(ValueError, match="1 samples per stream are not a multiple of the converter's down factor 147"):
        b.process_samples_at_device(4096, "s16", "stream", 1, 160, cap, None, "f32", "stream", 0, 0, None)
    with pytest.raises(ValueError, match="n_out 148 is not a multiple of the converter's up factor 147"):
        b.process_samples_at_device(None, "s16", "stream", 0, 0, None, 8192, "f32", "stream", 148, 160, play)
    # stream count and device, as for the resamplers
    with pytest.raises(ValueError, match="upsampler has 4 streams, the batch 3"):
        b.process_samples_at(frames, upsampler=_handle(CaptureConverter, 4, up=160, down=147))
    with pytest.raises(ValueError, match="downsampler has 2 streams, the batch 3"):
        b.process_samples_at(None, n_out=147, downsampler=_handle(PlaybackConverter, 2, up=147, down=160))
    with pytest.raises(ValueError, match="upsampler is on device 1, the batch on 0"):
        b.process_samples_at(frames, upsampler=_handle(CaptureConverter, 3, device=1, up=160, down=147))
    with pytest.raises(ValueError, match="downsampler is on device 2, the batch on 0"):
        b.process_samples_at(frames, upsampler=cap, n_out=147, downsampler=_handle(PlaybackConverter, 3, device=2, up=147, down=160))
    assert b.processDemodulationCallCount == 0 and b._L.calls == []      # nothing was counted as a call, the library never reached


def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "processor_ratecvt_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "processor_ratecvt_plan_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
