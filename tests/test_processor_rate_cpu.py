"""fskhip_processor_process_rate_host / _device (include/fskhip_next.h) without a GPU:
  * the symbols are declared in the header, exported and bound;
  * what they refuse first, through ctypes on libfskhip.so -- every return code and the whole fskhip_last_error() string, in the
    header's order: a null processor, an unknown format or layout (input side first), then a side that has a buffer and no handle.
    Behind the null check these read nothing of the processor, so a stand-in block of memory serves as one
    (tests/test_gpu_processor_rate.py goes on from there with live handles);
  * the Python argument checks of FSKProcessorBatch.process_samples_at on a batch without a device;
  * how the call chooses between its fused TX kernel and the two launches it replaces (csrc/fsk_processor_rate_plan.h), from a
    stand-alone program under AddressSanitizer and UBSan;
  * what the feature is for, through the model (tests/processor_rate_ref.py): a default-configuration payload modulated, decimated by
    6 into mu-law quanta of 160, interpolated quantum by quantum into the demodulator, comes back byte for byte -- which also fixes
    the quanta and the bytes the GPU loopback of test_gpu_processor_rate.py must reproduce."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import processor_rate_ref as model
from conftest import ROOT

OK, E_INVALID = 0, -1
F32, S16, MULAW, ALAW = 0, 1, 2, 3
STREAM, SAMPLE = 0, 1
S = 5
FORMS = (("fskhip_processor_process_rate_host", ()), ("fskhip_processor_process_rate_device", (None,)))


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
        assert "int %s(fskhip_processor *p, fskhip_resampler *up, fskhip_resampler *down, const void *" % name in hdr
        assert hasattr(raw, name) and name in _lib.SYMBOL_NAMES
    assert "hipError_t launch_processor_io_rate(" in launch
    assert L.fskhip_abi_version() == 8


@pytest.mark.parametrize("name,tail", FORMS)
def test_first_refusals_in_order(L, name, tail):
    fn = getattr(L, name)
    stand_in = np.full(4096, S, np.uint32)          # (never read before a handle has been seen; see the module's text)
    P = stand_in.ctypes.data
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data

    def call(p, up, down, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch):
        return fn(p, up, down, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch, 0, *tail)

    # 1. a null processor, before anything else is looked at
    refused(L, call(None, None, None, None, MULAW, SAMPLE, 0, 0, None, MULAW, SAMPLE, 0, 0), "null processor")
    refused(L, call(None, None, None, B + 1, 9, 9, 8, 0, B + 1, -1, 7, 8, 0), "null processor")
    # 2. an unknown format, then layout: the input side first, a NULL side included, before any handle is asked for
    refused(L, call(P, None, None, B + 1, 4, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown sample format 4" % name)
    refused(L, call(P, None, None, None, -1, STREAM, 0, 0, None, F32, STREAM, 0, 0), "%s: unknown sample format -1" % name)
    refused(L, call(P, None, None, B + 1, S16, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown layout 2" % name)
    refused(L, call(P, None, None, B + 1, S16, SAMPLE, 8, 0, B + 1, 5, 7, 8, 0), "%s: unknown sample format 5" % name)
    refused(L, call(P, None, None, B + 1, S16, SAMPLE, 8, 0, B + 1, ALAW, -1, 8, 0), "%s: unknown layout -1" % name)
    # 3. a side that has a buffer needs its handle: the input side first, before pitches and alignments
    refused(L, call(P, None, None, B + 1, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "%s: null up handle" % name)
    refused(L, call(P, None, None, None, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "%s: null down handle" % name)
    assert (stand_in == S).all() and not buf.any()


class _NoDevice:
    """FSKProcessorBatch.process_samples_at's argument checks need the stream count only: a batch without a processor behind it"""

    def __new__(cls, n_streams):
        from webaudio_modem_amd.processor import FSKProcessorBatch
        b = object.__new__(FSKProcessorBatch)
        b.n_streams, b.flags, b.processDemodulationCallCount, b._h = n_streams, 0, 0, None
        b.engine = type("NoEngine", (), {"device": 0})()
        return b


def _handle(kind, n_streams, device=0):
    """an Upsampler / Downsampler as the checks see one, without a device"""
    h = object.__new__(kind)
    h.n_streams, h.device, h._h = n_streams, device, None
    return h


def test_python_argument_checks():
    from webaudio_modem_amd import Downsampler, Upsampler
    b = _NoDevice(3)
    up, down = _handle(Upsampler, 3), _handle(Downsampler, 3)
    frames = np.zeros((8, 3), np.uint8)
    # process_samples' checks
    with pytest.raises(ValueError, match="unknown sample format 'pcm'"):
        b.process_samples_at(frames, in_fmt="pcm", upsampler=up)
    with pytest.raises(ValueError, match="unknown layout 'frames'"):
        b.process_samples_at(frames, in_layout="frames", upsampler=up)
    with pytest.raises(ValueError, match="unknown sample format 'ulaw'"):
        b.process_samples_at(None, n_out=8, out_fmt="ulaw", downsampler=down)
    with pytest.raises(ValueError, match="unknown layout 'planar'"):
        b.process_samples_at(frames, upsampler=up, n_out=8, out_layout="planar", downsampler=down)
    with pytest.raises(ValueError, match="format 'mulaw' takes uint8 samples, got int16"):
        b.process_samples_at(np.zeros((8, 3), np.int16), upsampler=up)
    with pytest.raises(ValueError, match="format 's16' takes int16 samples, got float32"):
        b.process_samples_at(np.zeros((3, 8), np.float32), in_fmt="s16", in_layout="stream", upsampler=up)
    with pytest.raises(ValueError, match="inputs must be"):
        b.process_samples_at(np.zeros((3, 8), np.uint8), upsampler=up)                       # rows handed over as frames
    with pytest.raises(ValueError, match="inputs must be"):
        b.process_samples_at(np.zeros((8, 3), np.int16), in_fmt="s16", in_layout="stream", upsampler=up)
    with pytest.raises(ValueError, match="samples must be a 2-D array"):
        b.process_samples_at(np.zeros((8, 3, 2), np.uint8), upsampler=up)
    # the handles: there, of the right kind, of the batch's stream count and device -- for a side that has samples
    with pytest.raises(ValueError, match="upsampler must be a filters.Upsampler, got NoneType"):
        b.process_samples_at(frames)
    with pytest.raises(ValueError, match="upsampler must be a filters.Upsampler, got Downsampler"):
        b.process_samples_at(frames, upsampler=down)
    with pytest.raises(ValueError, match="downsampler must be a filters.Downsampler, got NoneType"):
        b.process_samples_at(None, n_out=8)
    with pytest.raises(ValueError, match="downsampler must be a filters.Downsampler, got Upsampler"):
        b.process_samples_at(frames, upsampler=up, n_out=8, downsampler=up)
    with pytest.raises(ValueError, match="upsampler has 4 streams, the batch 3"):
        b.process_samples_at(frames, upsampler=_handle(Upsampler, 4))
    with pytest.raises(ValueError, match="downsampler has 2 streams, the batch 3"):
        b.process_samples_at(None, n_out=8, downsampler=_handle(Downsampler, 2))
    with pytest.raises(ValueError, match="upsampler is on device 1, the batch on 0"):
        b.process_samples_at(frames, upsampler=_handle(Upsampler, 3, device=1))
    with pytest.raises(ValueError, match="downsampler is on device 2, the batch on 0"):
        b.process_samples_at(frames, upsampler=up, n_out=8, downsampler=_handle(Downsampler, 3, device=2))
    with pytest.raises(ValueError, match="downsampler has 2 streams, the batch 3"):
        b.process_samples_at_device(None, "mulaw", "sample", 0, 3, None, 4096, "mulaw", "sample", 8, 3, _handle(Downsampler, 2))
    assert b.processDemodulationCallCount == 0      # nothing was counted as a call


def test_plan_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "processor_rate_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "processor_rate_plan_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_link_at_8_khz_through_the_model():
    """modulate -> / 6 -> mu-law quanta of 160 -> x 6 -> demodulate, quantum by quantum with carried delay lines: every byte, and
    the last of them before the signal's last quantum ends -- the trailing quantum adds none"""
    wire, got = model.link()
    n_sig = wire.shape[0] - model.TRAILING_QUANTA
    assert wire.shape[1:] == (model.QUANTUM,) and wire.dtype == np.uint8
    assert b"".join(got) == model.PAYLOAD
    assert b"".join(got[:n_sig]) == model.PAYLOAD and not any(got[n_sig:])
    assert (wire[-1][-32:] == 0xFF).all()           # the decimator has rung out: the wire ends in mu-law silence
    # the trailing quantum changes nothing in front of it
    assert model.link(trailing=0)[0].tobytes() == wire[:n_sig].tobytes()
