"""FilterDesign: the configure-time Butterworth designs the engine uses (reference
src/dsp/filters.ts:180-234), served by the C ABI so that Python, Node and the kernels' host
code share one implementation."""
import ctypes as C

from . import _lib


def _call(fn, *args):
    b = (C.c_double * 3)()
    a = (C.c_double * 3)()
    fn(*args, b, a)
    return {"b": list(b), "a": list(a)}


class FilterDesign:
    @staticmethod
    def butterworthLowpass(cutoffFreq, sampleRate):
        return _call(_lib.lib().fskhip_butterworth_lowpass, float(cutoffFreq), float(sampleRate))

    @staticmethod
    def butterworthHighpass(cutoffFreq, sampleRate):
        return _call(_lib.lib().fskhip_butterworth_highpass, float(cutoffFreq), float(sampleRate))

    @staticmethod
    def butterworthBandpass(centerFreq, bandwidth, sampleRate):
        return _call(_lib.lib().fskhip_butterworth_bandpass, float(centerFreq), float(bandwidth), float(sampleRate))

    # windowed-sinc FIR designs (filters.ts:243-314)
    @staticmethod
    def _sinc(fn, numTaps, *args):
        taps = (C.c_double * (int(numTaps) + 1))()
        n = fn(*[float(a) for a in args], int(numTaps), taps)
        if n < 0:
            _lib.check(n)
        return list(taps)[:n]

    @staticmethod
    def sincLowpass(cutoffFreq, sampleRate, numTaps):
        return FilterDesign._sinc(_lib.lib().fskhip_sinc_lowpass, numTaps, cutoffFreq, sampleRate)

    @staticmethod
    def sincHighpass(cutoffFreq, sampleRate, numTaps):
        return FilterDesign._sinc(_lib.lib().fskhip_sinc_highpass, numTaps, cutoffFreq, sampleRate)

    @staticmethod
    def sincBandpass(centerFreq, bandwidth, sampleRate, numTaps):
        return FilterDesign._sinc(_lib.lib().fskhip_sinc_bandpass, numTaps, centerFreq, bandwidth, sampleRate)


class FIRFilterBatch:
    """`new FIRFilter(coefficients)` (filters.ts:112-167) for n_streams streams on one GPU: `processBuffer` on a
    float32 [S, N] block, delay lines carried across calls, `reset`, `getCoefficients`."""

    def __init__(self, coefficients, n_streams=1, device=0, precision=_lib.PRECISION_F64):
        import numpy as np
        self._np = np
        self.coefficients = [float(c) for c in coefficients]
        if not self.coefficients:
            raise ValueError("FIR needs at least one coefficient")
        taps = (C.c_double * len(self.coefficients))(*self.coefficients)
        h = C.c_void_p()
        self._L = _lib.lib()
        _lib.check(self._L.fskhip_fir_create(device, taps, len(self.coefficients), n_streams, precision, C.byref(h)))
        self._h = h
        self.n_streams = n_streams

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_fir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def processBuffer(self, x):
        np = self._np
        x = np.ascontiguousarray(x, dtype=np.float32)
        single = x.ndim == 1
        if single:
            x = x[None, :]
        if x.shape[0] != self.n_streams:
            raise ValueError("input must be [n_streams, n]")
        out = np.empty_like(x)
        if x.shape[1]:
            _lib.check(self._L.fskhip_fir_process_host(self._h, x.ctypes.data, x.shape[1], x.shape[1], out.ctypes.data,
                                                       x.shape[1]))
        return out[0] if single else out

    def process_device(self, d_in, n, in_pitch, d_out, out_pitch, stream=None):
        _lib.check(self._L.fskhip_fir_process_device(self._h, d_in, n, in_pitch, d_out, out_pitch, stream))

    def reset(self, stream=-1):
        _lib.check(self._L.fskhip_fir_reset(self._h, stream))

    def getCoefficients(self):
        return list(self.coefficients)


class FIRFilter(FIRFilterBatch):
    """One FIRFilter with the reference's per-sample surface: process(x) is a batch of one sample."""

    def __init__(self, coefficients, device=0, precision=_lib.PRECISION_F64):
        super().__init__(coefficients, 1, device, precision)

    def process(self, x):
        return float(self.processBuffer(self._np.array([x], dtype=self._np.float32))[0])


class _RateHandle:
    """What the resamplers and the rate converters share: a handle of the library's `_PREFIX` family (include/fskhip_next.h:
    fskhip_resampler_* / fskhip_ratecvt_*) in `_h`, with n_streams and history beside it: close, reset, the history rows, and
    the two host calls' marshalling."""

    _PREFIX = None

    def _fn(self, name):
        return getattr(self._L, self._PREFIX + name)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=-1):
        _lib.check(self._fn("reset")(self._h, stream))

    def state(self):
        """the history rows, float32 [n_streams, history], oldest first (fskhip_*_state_get)"""
        st = self._np.zeros((self.n_streams, self.history), self._np.float32)
        _lib.check(self._fn("state_get")(self._h, st.ctypes.data))
        return st

    def set_state(self, state):
        """fskhip_*_state_set: rows as state() returns them, e.g. permuted by a remap's stream map"""
        st = self._np.ascontiguousarray(state, dtype=self._np.float32)
        if st.shape != (self.n_streams, self.history):
            raise ValueError("state must be [%d, %d]" % (self.n_streams, self.history))
        _lib.check(self._fn("state_set")(self._h, st.ctypes.data))

    def _widen(self, name, samples, fmt, layout, out_count, *tail):
        """the _host call `name` from samples as FSKEngine.demodulate_samples takes them to float32 [S, out_count(n)]; `tail`: what
        the call takes behind the pitches"""
        from .engine import sample_args
        x, code, lay, S, N, pitch = sample_args(samples, fmt, layout)
        if S != self.n_streams:
            raise ValueError("expected %d streams, got %d" % (self.n_streams, S))
        n_out = out_count(N)
        out = self._np.zeros((S, n_out), self._np.float32)
        if N:
            _lib.check(self._fn(name)(self._h, x.ctypes.data, code, lay, N, pitch, out.ctypes.data, max(n_out, 1), *tail))
        return out

    def _narrow(self, name, x, fmt, layout, lens, out, out_count, *tail):
        """the _host call `name` from float32 [S, n] to out_count(n) samples per stream as FSKEngine.modulate_samples returns them;
        `tail`: what the call takes behind the pitches"""
        from .engine import samples_out
        np = self._np
        x = np.asarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2 or x.shape[0] != self.n_streams:
            raise ValueError("input must be [n_streams, n]")
        if x.strides[1] != 4 and x.shape[1] > 1 or x.strides[0] % 4 or (x.shape[0] > 1 and x.strides[0] < 4 * x.shape[1]):
            x = np.ascontiguousarray(x)
        n = x.shape[1]
        out, code, lay, pitch = samples_out(fmt, layout, self.n_streams, out_count(n), out)
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.uint32)
        if ln is not None and ln.shape != (self.n_streams,):
            raise ValueError("need one length per stream")
        _lib.check(self._fn(name)(self._h, x.ctypes.data, n, max(x.strides[0] // 4 if x.shape[0] > 1 else n, n, 1),
                                  None if ln is None else ln.ctypes.data, out.ctypes.data, code, lay, pitch, *tail))
        return out


class _Resampler(_RateHandle):
    """What Upsampler and Downsampler share: an fskhip_resampler handle (include/fskhip_next.h) and its design; remap, snapshot
    and restore."""

    _PREFIX = "fskhip_resampler_"
    _DIRECTION = None

    def __init__(self, factor, n_streams, taps=None, low_rate=8000, device=0, precision=_lib.PRECISION_F32):
        import numpy as np
        self._np = np
        self.factor, self.n_streams, self.low_rate, self.device, self.precision = int(factor), int(n_streams), low_rate, device, precision
        if taps is None:
            if not 1 <= self.factor <= 32:
                raise ValueError("factor %d outside 1..32" % self.factor)
            # a Hamming-windowed sinc at 0.45 of the low rate (3 600 Hz at 8 kHz), 16 taps per phase and one
            taps = FilterDesign.sincLowpass(0.45 * low_rate, self.factor * low_rate, 16 * self.factor + 1)
            if self._DIRECTION == _lib.RESAMPLE_UP:
                taps = [t * float(self.factor) for t in taps]     # the stuffed zeros take 1 / factor of the level
        self.taps = [float(t) for t in taps]
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.fskhip_resampler_create(device, self._DIRECTION, self.factor, (C.c_double * max(1, len(self.taps)))(*self.taps),
                                                   len(self.taps), self.n_streams, precision, C.byref(h)))
        self._h = h
        self.history = int(self._L.fskhip_resampler_history(h))

    @classmethod
    def _adopt(cls, h, taps, factor, precision, device, low_rate):
        """an object of this class over a handle the library has created (remap, restore)"""
        import numpy as np
        nxt = cls.__new__(cls)
        nxt._np, nxt._L, nxt._h = np, _lib.lib(), h
        nxt.factor, nxt.low_rate, nxt.device, nxt.precision = int(factor), low_rate, device, int(precision)
        nxt.taps = [float(t) for t in taps]
        nxt.n_streams = int(nxt._L.fskhip_resampler_streams(h))
        nxt.history = int(nxt._L.fskhip_resampler_history(h))
        return nxt

    def remapped(self, stream_map):
        """fskhip_resampler_remap: a new object of this design whose stream i continues stream stream_map[i] of this one -- its
        history row, bit for bit -- or starts with a zero history where stream_map[i] is -1: the map the engine and the
        processor were remapped with.  The rows move on the device.  This object stays usable."""
        m = self._np.ascontiguousarray(stream_map, dtype=self._np.int64).reshape(-1)
        h = C.c_void_p()
        _lib.check(self._L.fskhip_resampler_remap(self._h, m.ctypes.data if len(m) else None, len(m), C.byref(h)))
        return self._adopt(h, self.taps, self.factor, self.precision, self.device, self.low_rate)

    def snapshot(self, streams=None):
        """fskhip_resampler_snapshot: the image of streams `streams` (None: all, in order) as `bytes` -- the design (direction,
        factor, precision, taps) and the history rows.  This object is read only and stays usable."""
        np = self._np
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int64).reshape(-1)
        n = self.n_streams if sel is None else len(sel)
        if sel is not None and not len(sel):
            sel = np.zeros(1, np.int64)   # (an empty selection, not "all": a non-null pointer with n = 0)
        sel_p = None if sel is None else sel.ctypes.data
        size = C.c_size_t(0)
        _lib.check(self._L.fskhip_resampler_snapshot_bytes(self._h, n, C.byref(size)))
        buf = np.zeros(max(size.value, 1), np.uint8)
        w = C.c_size_t(0)
        _lib.check(self._L.fskhip_resampler_snapshot(self._h, sel_p, n, buf.ctypes.data, size.value, C.byref(w)))
        return buf[:w.value].tobytes()

    @classmethod
    def from_snapshot(cls, snap, stream_map=None, device=0):
        """fskhip_resampler_restore: a new object on `device` from a snapshot() alone: stream i continues record stream_map[i]
        (-1: a zero history; None: every record, in order).  Upsampler and Downsampler refuse an image of the other direction."""
        import numpy as np
        from .engine import _blob
        info = resampler_snapshot_info(snap)
        if cls._DIRECTION is not None and info["direction"] != cls._DIRECTION:
            raise ValueError("the snapshot is of a resampler that goes %s, not %s" % (("up", "down")[info["direction"]], ("up", "down")[cls._DIRECTION]))
        kind = cls if cls._DIRECTION is not None else (Upsampler, Downsampler)[info["direction"]]
        b = _blob(snap)
        m = None if stream_map is None else np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        n = 0 if m is None else len(m)
        if m is not None and not n:
            m = np.zeros(1, np.int64)   # (an empty map, not "all": a non-null pointer with n = 0, which the library refuses)
        h = C.c_void_p()
        _lib.check(_lib.lib().fskhip_resampler_restore(device, b.ctypes.data, b.nbytes, None if m is None else m.ctypes.data, n, C.byref(h)))
        taps = np.frombuffer(b.tobytes(), dtype="<f8", count=info["n_taps"], offset=48)   # (the header is 48 bytes; the image has been validated)
        return kind._adopt(h, taps, info["factor"], info["precision"], device, None)


def resampler_snapshot_info(snap):
    """fskhip_resampler_snapshot_info_get: what a resampler snapshot holds -- n_streams (records), direction (0 up, 1 down), factor,
    n_taps, precision, history (floats per record) -- validated on the host, no device needed"""
    from .engine import _blob, _struct_dict
    b = _blob(snap)
    info = _lib.ResamplerSnapshotInfo()
    _lib.check(_lib.lib().fskhip_resampler_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


class Upsampler(_Resampler):
    """Capture samples at low_rate -> float32 [S, n * factor] at factor * low_rate, on the GPU: FIRFilterBatch(taps) over the
    zero-stuffed samples, evaluated polyphase, history carried across calls.  taps None: sincLowpass(0.45 * low_rate,
    factor * low_rate, 16 * factor + 1) times factor."""

    _DIRECTION = _lib.RESAMPLE_UP

    def process(self, samples, fmt=None, layout="stream"):
        """samples as FSKEngine.demodulate_samples takes them; returns float32 [S, n * factor]"""
        return self._widen("up_host", samples, fmt, layout, lambda n: n * self.factor)

    def process_device(self, d_src, fmt, layout, n_in, src_pitch, d_dst, dst_pitch, stream=None):
        """fskhip_resampler_up_device: device pointers (ints), asynchronous on `stream`"""
        from .engine import _sample_codes
        _lib.check(self._L.fskhip_resampler_up_device(self._h, d_src, *_sample_codes(fmt, layout, True), n_in, src_pitch, d_dst, dst_pitch, stream))


class Downsampler(_Resampler):
    """float32 [S, n] at factor * low_rate -> samples of a capture format at low_rate, on the GPU: FIRFilterBatch(taps) with every
    factor-th output kept, encoded; n must be a multiple of factor.  taps None: sincLowpass(0.45 * low_rate, factor * low_rate,
    16 * factor + 1)."""

    _DIRECTION = _lib.RESAMPLE_DOWN

    def process(self, x, fmt, layout="stream", lens=None, out=None):
        """x: float32 [S, n]; lens (or None): samples of stream s from lens[s] on read as 0.0.  Returns the samples as
        FSKEngine.modulate_samples does, [S, n / factor] or frames [n / factor, S]; `out`: the array to write into."""
        return self._narrow("down_host", x, fmt, layout, lens, out, lambda n: n // self.factor)

    def process_device(self, d_src, n_in, src_pitch, d_lens, d_dst, fmt, layout, dst_pitch, stream=None):
        """fskhip_resampler_down_device: device pointers (ints), asynchronous on `stream`"""
        from .engine import _sample_codes
        _lib.check(self._L.fskhip_resampler_down_device(self._h, d_src, n_in, src_pitch, d_lens, d_dst, *_sample_codes(fmt, layout, True), dst_pitch, stream))

    def low_rate_length(self, n):
        """low rate samples that hold a signal of n samples and the filter's ringing behind it"""
        return (int(n) + len(self.taps) - 1 + self.factor - 1) // self.factor


class _RateConverter(_RateHandle):
    """What CaptureConverter and PlaybackConverter share: an fskhip_ratecvt handle (include/fskhip_next.h) that converts in_rate to
    out_rate by up / down, the rates over their gcd, and its design."""

    _PREFIX = "fskhip_ratecvt_"
    _DIRECTION = None
    MAX_FACTOR, MAX_TAPS = 256, 4096

    @staticmethod
    def ratio(in_rate, out_rate):
        """(up, down) for in_rate -> out_rate: the rates, whole numbers, over their gcd"""
        from math import gcd
        i, o = int(in_rate), int(out_rate)
        if i != in_rate or o != out_rate or i < 1 or o < 1:
            raise ValueError("rates must be positive whole numbers, got %r and %r" % (in_rate, out_rate))
        g = gcd(i, o)
        return o // g, i // g

    @classmethod
    def default_taps(cls, in_rate, out_rate):
        """the design of taps=None: a Hamming-windowed sinc at 0.45 of the lower rate, designed at up * in_rate, 16 taps per phase of
        the larger factor and one, times up (the stuffed zeros take 1 / up of the level): 2 561 taps and 19 845 Hz for
        44.1 kHz <-> 48 kHz"""
        up, down = cls.ratio(in_rate, out_rate)
        n = 16 * max(up, down) + 1
        if n > cls.MAX_TAPS:
            raise ValueError("the default design for %d / %d needs %d taps, the limit is %d" % (up, down, n, cls.MAX_TAPS))
        return [t * float(up) for t in FilterDesign.sincLowpass(0.45 * min(in_rate, out_rate), float(up) * in_rate, n)]

    def __init__(self, in_rate, out_rate, n_streams, taps=None, device=0, precision=_lib.PRECISION_F32):
        import numpy as np
        self._np = np
        self.in_rate, self.out_rate, self.n_streams, self.device, self.precision = in_rate, out_rate, int(n_streams), device, precision
        self.up, self.down = self.ratio(in_rate, out_rate)
        if taps is None:
            taps = self.default_taps(in_rate, out_rate)
        self.taps = [float(t) for t in taps]
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.fskhip_ratecvt_create(device, self._DIRECTION, self.up, self.down, (C.c_double * max(1, len(self.taps)))(*self.taps),
                                                 len(self.taps), self.n_streams, precision, C.byref(h)))
        self._h = h
        self.history = int(self._L.fskhip_ratecvt_history(h))

    def out_count(self, n_in):
        """samples per stream a call with n_in per stream (a multiple of `down`) writes"""
        return int(n_in) // self.down * self.up

    @property
    def position(self):
        """fskhip_ratecvt_position: the inputs taken since the last period boundary, 0 .. down - 1, one number for all streams; 0
        at creation and after reset(), moved on by process_any.  Settable (fskhip_ratecvt_position_set): with state() / set_state()
        the by-hand carry of a handle"""
        return int(self._L.fskhip_ratecvt_position(self._h))

    @position.setter
    def position(self, pos):
        if not 0 <= int(pos) < self.down:
            raise ValueError("position %d outside 0..%d" % (int(pos), self.down - 1))
        _lib.check(self._L.fskhip_ratecvt_position_set(self._h, int(pos)))

    def out_count_any(self, n_in):
        """samples per stream process_any writes for n_in per stream from the current position (fskhip_ratecvt_out_count_any)"""
        return int(self._L.fskhip_ratecvt_out_count_any(self._h, int(n_in)))

    def in_count_any(self, n_out):
        """the fewest samples per stream for which process_any writes at least n_out from the current position -- exactly n_out
        where up <= down (fskhip_ratecvt_in_count_any)"""
        return int(self._L.fskhip_ratecvt_in_count_any(self._h, int(n_out)))

    @classmethod
    def _adopt(cls, h, taps, up, down, precision, device, in_rate, out_rate):
        """an object of this class over a handle the library has created (remap, restore)"""
        import numpy as np
        nxt = cls.__new__(cls)
        nxt._np, nxt._L, nxt._h = np, _lib.lib(), h
        nxt.up, nxt.down, nxt.in_rate, nxt.out_rate, nxt.device, nxt.precision = int(up), int(down), in_rate, out_rate, device, int(precision)
        nxt.taps = [float(t) for t in taps]
        nxt.n_streams = int(nxt._L.fskhip_ratecvt_streams(h))
        nxt.history = int(nxt._L.fskhip_ratecvt_history(h))
        return nxt

    def remapped(self, stream_map):
        """fskhip_ratecvt_remap: a new object of this design, at this position, whose stream i continues stream stream_map[i] of
        this one -- its history row, bit for bit -- or starts with a zero history where stream_map[i] is -1 (a stream that has
        received zeros since the last period boundary): the map the engine and the processor were remapped with.  The rows move on
        the device.  This object stays usable."""
        m = self._np.ascontiguousarray(stream_map, dtype=self._np.int64).reshape(-1)
        h = C.c_void_p()
        _lib.check(self._L.fskhip_ratecvt_remap(self._h, m.ctypes.data if len(m) else None, len(m), C.byref(h)))
        return self._adopt(h, self.taps, self.up, self.down, self.precision, self.device, self.in_rate, self.out_rate)

    def snapshot(self, streams=None):
        """fskhip_ratecvt_snapshot: the image of streams `streams` (None: all, in order) as `bytes` -- the design (direction, up,
        down, precision, taps), the position and the history rows.  This object is read only and stays usable."""
        np = self._np
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int64).reshape(-1)
        n = self.n_streams if sel is None else len(sel)
        if sel is not None and not len(sel):
            sel = np.zeros(1, np.int64)   # (an empty selection, not "all": a non-null pointer with n = 0)
        sel_p = None if sel is None else sel.ctypes.data
        size = C.c_size_t(0)
        _lib.check(self._L.fskhip_ratecvt_snapshot_bytes(self._h, n, C.byref(size)))
        buf = np.zeros(max(size.value, 1), np.uint8)
        w = C.c_size_t(0)
        _lib.check(self._L.fskhip_ratecvt_snapshot(self._h, sel_p, n, buf.ctypes.data, size.value, C.byref(w)))
        return buf[:w.value].tobytes()

    @classmethod
    def from_snapshot(cls, snap, stream_map=None, device=0, in_rate=None, out_rate=None):
        """fskhip_ratecvt_restore: a new object on `device` from a snapshot() alone, at the image's position: stream i continues
        record stream_map[i] (-1: a zero history; None: every record, in order).  CaptureConverter and PlaybackConverter refuse an
        image of the other direction; _RateConverter picks the class from the image.  An image knows up and down, not the rates:
        without them in_rate / out_rate are down / up; rates that do not reduce to the image's ratio are a ValueError."""
        import numpy as np
        from .engine import _blob
        info = ratecvt_snapshot_info(snap)
        names = ("capture", "playback")
        if cls._DIRECTION is not None and info["direction"] != cls._DIRECTION:
            raise ValueError("the snapshot is of a rate converter for %s, not %s" % (names[info["direction"]], names[cls._DIRECTION]))
        kind = cls if cls._DIRECTION is not None else (CaptureConverter, PlaybackConverter)[info["direction"]]
        if (in_rate is None) != (out_rate is None):
            raise ValueError("give both in_rate and out_rate, or neither")
        if in_rate is None:
            in_rate, out_rate = info["down"], info["up"]
        elif cls.ratio(in_rate, out_rate) != (info["up"], info["down"]):
            raise ValueError("%r -> %r is %d / %d, the snapshot converts by %d / %d" % ((in_rate, out_rate) + cls.ratio(in_rate, out_rate) + (info["up"], info["down"])))
        b = _blob(snap)
        m = None if stream_map is None else np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        n = 0 if m is None else len(m)
        if m is not None and not n:
            m = np.zeros(1, np.int64)   # (an empty map, not "all": a non-null pointer with n = 0, which the library refuses)
        h = C.c_void_p()
        _lib.check(_lib.lib().fskhip_ratecvt_restore(device, b.ctypes.data, b.nbytes, None if m is None else m.ctypes.data, n, C.byref(h)))
        taps = np.frombuffer(b, dtype="<f8", count=info["n_taps"], offset=64)   # (the header is 64 bytes; the image has been validated)
        return kind._adopt(h, taps, info["up"], info["down"], info["precision"], device, in_rate, out_rate)


def ratecvt_snapshot_info(snap):
    """fskhip_ratecvt_snapshot_info_get: what a rate converter snapshot holds -- n_streams (records), direction (0 capture,
    1 playback), up, down, n_taps, precision, history (floats per record), position -- validated on the host, no device needed"""
    from .engine import _blob, _struct_dict
    b = _blob(snap)
    info = _lib.RatecvtSnapshotInfo()
    _lib.check(_lib.lib().fskhip_ratecvt_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


class CaptureConverter(_RateConverter):
    """Capture samples at in_rate -> float32 [S, n / down * up] at out_rate, on the GPU (44.1 kHz in front of a 48 kHz engine:
    up / down = 160 / 147): FIRFilterBatch(taps) over the samples zero-stuffed by `up` with every `down`-th output kept, evaluated
    polyphase, history carried across calls; n must be a multiple of `down`."""

    _DIRECTION = _lib.RATECVT_CAPTURE

    def process(self, samples, fmt=None, layout="stream"):
        """samples as FSKEngine.demodulate_samples takes them; returns float32 [S, n / down * up]"""
        return self._widen("capture_host", samples, fmt, layout, self.out_count)

    def process_device(self, d_src, fmt, layout, n_in, src_pitch, d_dst, dst_pitch, stream=None):
        """fskhip_ratecvt_capture_device: device pointers (ints), asynchronous on `stream`"""
        from .engine import _sample_codes
        _lib.check(self._L.fskhip_ratecvt_capture_device(self._h, d_src, *_sample_codes(fmt, layout, True), n_in, src_pitch, d_dst, dst_pitch, stream))

    def process_any(self, samples, fmt=None, layout="stream"):
        """process() for any number of samples per stream, from the handle's position: returns float32 [S, out_count_any(n)] --
        possibly no columns -- and moves the position on"""
        return self._widen("capture_any_host", samples, fmt, layout, self.out_count_any, None)

    def process_any_device(self, d_src, fmt, layout, n_in, src_pitch, d_dst, dst_pitch, stream=None):
        """fskhip_ratecvt_capture_any_device: device pointers (ints), asynchronous on `stream`; returns the floats written per stream"""
        from .engine import _sample_codes
        n_out = C.c_size_t(0)
        _lib.check(self._L.fskhip_ratecvt_capture_any_device(self._h, d_src, *_sample_codes(fmt, layout, True), n_in, src_pitch, d_dst, dst_pitch, C.byref(n_out), stream))
        return n_out.value


class PlaybackConverter(_RateConverter):
    """float32 [S, n] at in_rate -> samples of a capture format at out_rate, on the GPU (a 48 kHz engine in front of a 44.1 kHz
    sound card: up / down = 147 / 160): the same filter, encoded; n must be a multiple of `down`."""

    _DIRECTION = _lib.RATECVT_PLAYBACK

    def process(self, x, fmt, layout="stream", lens=None, out=None):
        """x: float32 [S, n]; lens (or None): samples of stream s from lens[s] on read as 0.0.  Returns the samples as
        FSKEngine.modulate_samples does, [S, n / down * up] or frames [n / down * up, S]; `out`: the array to write into."""
        return self._narrow("playback_host", x, fmt, layout, lens, out, self.out_count)

    def process_device(self, d_src, n_in, src_pitch, d_lens, d_dst, fmt, layout, dst_pitch, stream=None):
        """fskhip_ratecvt_playback_device: device pointers (ints), asynchronous on `stream`"""
        from .engine import _sample_codes
        _lib.check(self._L.fskhip_ratecvt_playback_device(self._h, d_src, n_in, src_pitch, d_lens, d_dst, *_sample_codes(fmt, layout, True), dst_pitch, stream))

    def process_any(self, x, fmt, layout="stream", lens=None, out=None):
        """process() for any number of floats per stream, from the handle's position: returns [S, out_count_any(n)] samples or
        frames [out_count_any(n), S] -- possibly none -- and moves the position on; lens count from the call's first input"""
        return self._narrow("playback_any_host", x, fmt, layout, lens, out, self.out_count_any, None)

    def process_any_device(self, d_src, n_in, src_pitch, d_lens, d_dst, fmt, layout, dst_pitch, stream=None):
        """fskhip_ratecvt_playback_any_device: device pointers (ints), asynchronous on `stream`; returns the samples written per stream"""
        from .engine import _sample_codes
        n_out = C.c_size_t(0)
        _lib.check(self._L.fskhip_ratecvt_playback_any_device(self._h, d_src, n_in, src_pitch, d_lens, d_dst, *_sample_codes(fmt, layout, True), dst_pitch,
                                                              C.byref(n_out), stream))
        return n_out.value

    def out_length(self, n):
        """output samples that can be non-zero for a signal of n input samples: the signal and the filter's ringing behind it"""
        n = int(n)
        return ((n - 1) * self.up + len(self.taps) - 1) // self.down + 1 if n else 0


class IIRFilterBatch:
    """`new IIRFilter(b, a)` (filters.ts:8-106) for n_streams streams on one GPU: `processBuffer` on a float32 [S, N]
    block (Float32Array in, Float32Array out), `processSamples` on a float64 block (what `process(x)` returns sample by
    sample, nothing rounded to float), histories carried across calls, `reset`, `getCoefficients` (normalised by a[0]).
    The constructor's three errors are the reference's (filters.ts:19-21), raised as ValueError with its messages."""

    def __init__(self, b, a, n_streams=1, device=0, precision=_lib.PRECISION_F64):
        import numpy as np
        self._np = np
        b = [float(v) for v in (b if b is not None else [])]
        a = [float(v) for v in (a if a is not None else [])]
        # filters.ts:19-21 (checked here too so that the errors do not need a GPU; the library checks again)
        if len(b) == 0:
            raise ValueError("Feedforward coefficients (b) cannot be empty")
        if len(a) == 0:
            raise ValueError("Feedback coefficients (a) cannot be empty")
        if a[0] == 0:
            raise ValueError("First feedback coefficient (a[0]) cannot be zero")
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.fskhip_iir_create(device, (C.c_double * len(b))(*b), len(b), (C.c_double * len(a))(*a), len(a),
                                             n_streams, precision, C.byref(h)))
        self._h = h
        self.n_streams = n_streams

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_iir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, x, dtype, fn):
        np = self._np
        x = np.ascontiguousarray(x, dtype=dtype)
        single = x.ndim == 1
        if single:
            x = x[None, :]
        if x.shape[0] != self.n_streams:
            raise ValueError("input must be [n_streams, n]")
        out = np.empty_like(x)
        if x.shape[1]:
            _lib.check(fn(self._h, x.ctypes.data, x.shape[1], x.shape[1], out.ctypes.data, x.shape[1]))
        return out[0] if single else out

    def processBuffer(self, x):
        return self._run(x, self._np.float32, self._L.fskhip_iir_process_host)

    def processSamples(self, x):
        return self._run(x, self._np.float64, self._L.fskhip_iir_process_f64_host)

    def process_device(self, d_in, n, in_pitch, d_out, out_pitch, stream=None):
        _lib.check(self._L.fskhip_iir_process_device(self._h, d_in, n, in_pitch, d_out, out_pitch, stream))

    def reset(self, stream=-1):
        _lib.check(self._L.fskhip_iir_reset(self._h, stream))

    def getCoefficients(self):
        b, a = (C.c_double * 9)(), (C.c_double * 9)()
        nb, na = C.c_uint32(), C.c_uint32()
        _lib.check(self._L.fskhip_iir_get_coefficients(self._h, b, C.byref(nb), a, C.byref(na)))
        return {"b": list(b[:nb.value]), "a": list(a[:na.value])}


class IIRFilter(IIRFilterBatch):
    """One IIRFilter with the reference's per-sample surface: process(x) takes and returns a number."""

    def __init__(self, b, a, device=0, precision=_lib.PRECISION_F64):
        super().__init__(b, a, 1, device, precision)

    def process(self, x):
        return float(self.processSamples(self._np.array([x], dtype=self._np.float64))[0])


class FilterFactory:
    """FilterFactory.createIIR* (filters.ts:325-344) and createFIR* (346-368)."""

    @staticmethod
    def createIIRLowpass(cutoffFreq, sampleRate, **kw):
        d = FilterDesign.butterworthLowpass(cutoffFreq, sampleRate)
        return IIRFilter(d["b"], d["a"], **kw)

    @staticmethod
    def createIIRHighpass(cutoffFreq, sampleRate, **kw):
        d = FilterDesign.butterworthHighpass(cutoffFreq, sampleRate)
        return IIRFilter(d["b"], d["a"], **kw)

    @staticmethod
    def createIIRBandpass(centerFreq, bandwidth, sampleRate, **kw):
        d = FilterDesign.butterworthBandpass(centerFreq, bandwidth, sampleRate)
        return IIRFilter(d["b"], d["a"], **kw)

    @staticmethod
    def createFIRLowpass(cutoffFreq, sampleRate, numTaps=51, **kw):
        return FIRFilter(FilterDesign.sincLowpass(cutoffFreq, sampleRate, numTaps), **kw)

    @staticmethod
    def createFIRHighpass(cutoffFreq, sampleRate, numTaps=51, **kw):
        return FIRFilter(FilterDesign.sincHighpass(cutoffFreq, sampleRate, numTaps), **kw)

    @staticmethod
    def createFIRBandpass(centerFreq, bandwidth, sampleRate, numTaps=51, **kw):
        return FIRFilter(FilterDesign.sincBandpass(centerFreq, bandwidth, sampleRate, numTaps), **kw)
