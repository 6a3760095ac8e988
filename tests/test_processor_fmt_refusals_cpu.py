"""fskhip_processor_process_fmt_host / _device (include/fskhip_next.h): what they refuse before any device call, through ctypes on
libfskhip.so -- every return code and the whole fskhip_last_error() string, in the header's order: a null processor, an unknown
format or layout (input side first), a pitch that is too small, a pointer misaligned for its element.  No device is needed: behind
the null check the refusals read one word of the processor, n_streams, so a stand-in block of memory whose every 32-bit word is 5
serves as a processor of five streams (tests/test_gpu_processor_fmt.py repeats them on a real one).  Also the Python argument
checks of FSKProcessorBatch.process_samples, which come before the library is called."""
import ctypes as C

import numpy as np
import pytest

OK, E_INVALID = 0, -1
F32, S16, MULAW, ALAW = 0, 1, 2, 3
STREAM, SAMPLE = 0, 1
S = 5


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    return _lib.lib()


def refused(L, rc, text):
    assert (rc, L.fskhip_last_error().decode()) == (E_INVALID, text)


FORMS = (("fskhip_processor_process_fmt_host", (), "in", "out"), ("fskhip_processor_process_fmt_device", (None,), "d_in", "d_out"))


@pytest.mark.parametrize("name,tail,in_name,out_name", FORMS)
def test_refusals_in_order(L, name, tail, in_name, out_name):
    fn = getattr(L, name)
    stand_in = np.full(4096, S, np.uint32)          # (read for n_streams only; see the module's text)
    P = stand_in.ctypes.data
    buf = np.zeros(256, np.uint8)
    B = buf.ctypes.data                             # B + 1 is odd and B + 2 no multiple of 4
    assert B % 4 == 0

    def call(p, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch):
        return fn(p, d_in, in_fmt, in_lay, n_in, in_pitch, d_out, out_fmt, out_lay, n_out, out_pitch, 0, *tail)

    # 1. a null processor, before anything else is looked at
    refused(L, call(None, None, F32, STREAM, 0, 0, None, F32, STREAM, 0, 0), "null processor")
    refused(L, call(None, B + 1, 9, 9, 8, 0, B + 1, -1, 7, 8, 0), "null processor")
    # 2. an unknown format or layout: the input side first, the format before the layout, a NULL side included
    refused(L, call(P, B + 1, 4, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown sample format 4" % name)
    refused(L, call(P, None, -1, STREAM, 0, 0, None, F32, STREAM, 0, 0), "%s: unknown sample format -1" % name)
    refused(L, call(P, B + 1, S16, 2, 8, 0, B + 1, -1, 7, 8, 0), "%s: unknown layout 2" % name)
    refused(L, call(P, B + 1, S16, SAMPLE, 8, 0, B + 1, 5, 7, 8, 0), "%s: unknown sample format 5" % name)
    refused(L, call(P, B + 1, S16, SAMPLE, 8, 0, B + 1, ALAW, -1, 8, 0), "%s: unknown layout -1" % name)
    # 3. a pitch that is too small, of a side that is there: in before out, before any alignment
    refused(L, call(P, B + 1, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "in_pitch 7 < n_in 8")
    refused(L, call(P, B + 1, MULAW, SAMPLE, 8, S - 1, B + 1, S16, STREAM, 8, 7), "in frame pitch 4 < n_streams 5")
    refused(L, call(P, None, S16, STREAM, 8, 7, B + 1, S16, STREAM, 8, 7), "out_pitch 7 < n_out 8")
    refused(L, call(P, B + 1, S16, SAMPLE, 3, S, B + 1, ALAW, SAMPLE, 8, 0), "out frame pitch 0 < n_streams 5")
    refused(L, call(P, B + 1, F32, STREAM, 0, 0, B + 1, F32, SAMPLE, 0, S - 1), "out frame pitch 4 < n_streams 5")
    # 4. a pointer misaligned for its element: in before out; bytes have no alignment
    refused(L, call(P, B + 1, S16, STREAM, 8, 8, B + 1, S16, STREAM, 8, 8), "%s is not aligned to its element size" % in_name)
    refused(L, call(P, B + 2, F32, SAMPLE, 8, S, B + 1, S16, STREAM, 8, 8), "%s is not aligned to its element size" % in_name)
    refused(L, call(P, B + 2, S16, SAMPLE, 8, S, B + 1, S16, STREAM, 8, 8), "%s is not aligned to its element size" % out_name)
    refused(L, call(P, B + 1, MULAW, STREAM, 8, 8, B + 2, F32, SAMPLE, 8, S), "%s is not aligned to its element size" % out_name)
    refused(L, call(P, None, S16, STREAM, 8, 8, B + 1, S16, SAMPLE, 0, S), "%s is not aligned to its element size" % out_name)
    assert (stand_in == S).all() and not buf.any()


def test_symbols_are_declared_exported_and_bound(L):
    import os
    from webaudio_modem_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fskhip_next.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("fskhip_processor_process_fmt_host", "fskhip_processor_process_fmt_device"):
        assert "int %s(fskhip_processor *p, const void *" % name in hdr
        assert hasattr(raw, name) and name in _lib.SYMBOL_NAMES
    assert L.fskhip_abi_version() == 8


class _NoDevice:
    """FSKProcessorBatch.process_samples's argument checks need the stream count only: a batch without a processor behind it"""

    def __new__(cls, n_streams):
        from webaudio_modem_amd.processor import FSKProcessorBatch
        b = object.__new__(FSKProcessorBatch)
        b.n_streams, b.flags, b.processDemodulationCallCount, b._h = n_streams, 0, 0, None
        return b


def test_python_argument_checks():
    b = _NoDevice(3)
    with pytest.raises(ValueError, match="unknown sample format 'pcm'"):
        b.process_samples(np.zeros((3, 8), np.float32), in_fmt="pcm")
    with pytest.raises(ValueError, match="unknown layout 'frames'"):
        b.process_samples(np.zeros((3, 8), np.float32), in_layout="frames")
    with pytest.raises(ValueError, match="unknown sample format 'ulaw'"):
        b.process_samples(None, n_out=8, out_fmt="ulaw")
    with pytest.raises(ValueError, match="unknown layout 'planar'"):
        b.process_samples(None, n_out=8, out_layout="planar")
    # wrong dtype for the format
    with pytest.raises(ValueError, match="format 's16' takes int16 samples, got float32"):
        b.process_samples(np.zeros((3, 8), np.float32), in_fmt="s16")
    with pytest.raises(ValueError, match="format 'mulaw' takes uint8 samples, got int16"):
        b.process_samples(np.zeros((8, 3), np.int16), in_fmt="mulaw", in_layout="sample")
    with pytest.raises(ValueError, match="format 'f32' takes float32 samples, got float64"):
        b.process_samples(np.zeros((3, 8)))
    # wrong shape for the layout
    with pytest.raises(ValueError, match="inputs must be"):
        b.process_samples(np.zeros((8, 3), np.int16), in_fmt="s16")                        # frames handed over as rows
    with pytest.raises(ValueError, match="inputs must be"):
        b.process_samples(np.zeros((3, 8), np.uint8), in_fmt="alaw", in_layout="sample")   # rows handed over as frames
    with pytest.raises(ValueError, match="samples must be a 2-D array"):
        b.process_samples(np.zeros((3, 8, 2), np.int16), in_fmt="s16")
    with pytest.raises(ValueError, match="unknown sample format 'ulaw'"):
        b.process_samples(np.zeros((3, 8), np.float32), n_out=8, out_fmt="ulaw")           # inputs that are fine, an output format that is none
    with pytest.raises(ValueError, match="unknown layout 'planar'"):
        b.process_samples(np.zeros((3, 8), np.float32), n_out=8, out_layout="planar")
    assert b.processDemodulationCallCount == 0      # nothing was counted as a call
