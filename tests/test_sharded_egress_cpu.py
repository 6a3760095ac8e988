"""FSKEngineSharded.modulate_samples (webaudio_modem_amd/sharded.py) on the CPU with a stand-in engine: every shard is handed its
row block of ONE stream-major array, or its column block of ONE array of interleaved frames at the full frame pitch -- views, no
copies -- and the lengths come back in stream order."""
import numpy as np
import pytest

import webaudio_modem_amd as wm
from webaudio_modem_amd.engine import samples_out


class FakeEngine:
    """Modulates nothing: fills what it is handed with its device number and records where that was."""

    def __init__(self, count, cfg, dev, prec):
        self.count, self.dev = count, dev
        self.calls = []

    def modulated_length(self, n_bytes):
        return 10 * n_bytes + 3

    def modulate_samples(self, payloads, fmt, layout="stream", n_per_stream=None, out=None):
        assert len(payloads) == self.count and out is not None
        arr, code, lay, pitch = samples_out(fmt, layout, self.count, n_per_stream, out)
        assert arr is out                                     # the shard works on the caller's memory
        self.calls.append((code, lay, n_per_stream, arr.ctypes.data, pitch, arr.shape))
        arr[...] = self.dev
        return arr, np.array([len(p) + 100 * self.dev for p in payloads], np.uint32)

    def close(self):
        pass


def make(count, cfg, dev, prec):
    return FakeEngine(count, cfg, dev, prec)


@pytest.mark.parametrize("fmt,dtype,code", [("s16", np.int16, 1), ("mulaw", np.uint8, 2), ("f32", np.float32, 0)])
def test_row_blocks_and_column_blocks_of_one_array(fmt, dtype, code):
    S, devs = 10, [5, 7, 9]                                    # shards of 4, 3 and 3 streams
    eng = wm.FSKEngineSharded(S, {}, devices=devs, engine_factory=make)
    payloads = [b"x" * (s + 1) for s in range(S)]
    firsts = [f for f, _, _ in eng.shards]
    counts = [c for _, c, _ in eng.shards]
    assert counts == [4, 3, 3]
    isz = np.dtype(dtype).itemsize

    out, lens = eng.modulate_samples(payloads, fmt)            # stream-major, n from the longest payload
    n = 10 * S + 3
    assert out.shape == (S, n) and out.dtype == dtype
    for e, first, count in zip(eng.engines, firsts, counts):
        assert e.calls[-1] == (code, 0, n, out.ctypes.data + first * n * isz, n, (count, n))
        assert (out[first:first + count] == e.dev).all()
    assert lens.dtype == np.uint32 and lens.tolist() == [s + 1 + 100 * devs[eng.locate(s)[0]] for s in range(S)]

    out, lens = eng.modulate_samples(payloads, fmt, layout="sample", n_per_stream=6)
    assert out.shape == (6, S)
    for e, first, count in zip(eng.engines, firsts, counts):   # its first column's address and the FULL frame pitch
        assert e.calls[-1] == (code, 1, 6, out.ctypes.data + first * isz, S, (6, count))
        assert (out[:, first:first + count] == e.dev).all()

    # into the caller's array, itself a column range of wider frames: the columns beyond stay untouched
    wide = np.full((6, S + 3), 99, dtype)
    got, _ = eng.modulate_samples(payloads, fmt, layout="sample", n_per_stream=6, out=wide[:, :S])
    assert got.ctypes.data == wide.ctypes.data and (wide[:, S:] == 99).all() and not (wide[:, :S] == 99).any()
    for e, first, count in zip(eng.engines, firsts, counts):
        assert e.calls[-1][3:5] == (wide.ctypes.data + first * isz, S + 3)
    with pytest.raises(ValueError, match="one payload per stream"):
        eng.modulate_samples(payloads[:-1], fmt)
    with pytest.raises(ValueError, match="shape"):
        eng.modulate_samples(payloads, fmt, layout="sample", n_per_stream=6, out=np.zeros((S, 6), dtype))
    eng.close()
