"""Batch FSK engine: Python host side above the C ABI (include/fskhip.h).

`FSKEngine` holds S independent FSKCore-equivalent streams on one MI355X.  Names and argument
meaning follow the reference's FSKCore (src/modems/fsk.ts): configure-time `FSKConfig` dicts
with the reference's field names, `demodulate_data` / `modulate_data` == demodulateData /
modulateData applied to every stream, `reset`, `get_status`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Config, Status, FskHipError, PRECISION_F32, PRECISION_F64, DEMOD_WRITEBACK_AGC  # noqa: F401

PARITY = {"none": 0, "even": 1, "odd": 2}

# DEFAULT_FSK_CONFIG (fsk.ts:19-33)
DEFAULT_FSK_CONFIG = dict(
    sampleRate=48000, baudRate=1200, markFrequency=1650, spaceFrequency=1850,
    preamblePattern=[0x55, 0x55], sfdPattern=[0x7E], startBits=1, stopBits=1, parity="none",
    syncThreshold=0.85, agcEnabled=True, preFilterBandwidth=800, adaptiveThreshold=True)


def make_config(cfg=None):
    """Merge a (partial) FSKConfig dict over DEFAULT_FSK_CONFIG, like configure() does (fsk.ts:134)."""
    merged = dict(DEFAULT_FSK_CONFIG)
    merged.update(cfg or {})
    c = Config()
    for k, v in merged.items():
        if k == "preamblePattern":
            if len(v) > _lib.MAX_PATTERN_BYTES:
                raise ValueError("preamblePattern longer than %d bytes" % _lib.MAX_PATTERN_BYTES)
            c.preambleLen = len(v)
            for i, b in enumerate(v):
                c.preamblePattern[i] = int(b)
        elif k == "sfdPattern":
            if len(v) > _lib.MAX_PATTERN_BYTES:
                raise ValueError("sfdPattern longer than %d bytes" % _lib.MAX_PATTERN_BYTES)
            c.sfdLen = len(v)
            for i, b in enumerate(v):
                c.sfdPattern[i] = int(b)
        elif k == "parity":
            c.parity = PARITY[v] if isinstance(v, str) else int(v)
        elif k in ("agcEnabled", "adaptiveThreshold"):
            setattr(c, k, 1 if v else 0)
        elif hasattr(c, k):
            setattr(c, k, v)
        else:
            raise KeyError("unknown FSKConfig field %r" % k)
    return c, merged


def _status_dict(st):
    return {
        "ready": bool(st.ready), "frameStarted": bool(st.frameStarted),
        "globalSampleCounter": int(st.globalSampleCounter), "receivedBitsLength": int(st.receivedBitsLength),
        "byteBufferLength": int(st.byteBufferLength), "demodulationCalls": int(st.demodulationCalls),
        "syncDetections": int(st.syncDetections), "silenceThreshold": float(st.silenceThreshold),
        "totalSamplesProcessed": int(st.totalSamplesProcessed),
        "agcGain": float(st.agcGain), "eodCount": int(st.eodCount),
    }


class _PinnedBlock:
    """owner of one fskhip_host_alloc allocation (freed when the last array viewing it is collected)"""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _lib.check(_lib.lib().fskhip_host_alloc(nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().fskhip_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float32):
    """numpy array in page-locked host memory (fskhip_host_alloc): the buffer to hand to demodulate_data /
    modulate_data when the PCIe copies should overlap the kernels (include/fskhip.h, fskhip_demodulate_host)."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    blk = _PinnedBlock(max(1, n * dt.itemsize))
    buf = (C.c_char * blk.nbytes).from_address(blk.ptr)
    arr = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    _PINNED_OWNERS[id(buf)] = blk          # keep the block alive as long as the ctypes buffer is
    import weakref
    weakref.finalize(buf, _PINNED_OWNERS.pop, id(buf), None)
    return arr


_PINNED_OWNERS = {}

_PARITY_NAME = {v: k for k, v in PARITY.items()}


def _blob(blob):
    """a snapshot as a contiguous uint8 array (bytes, bytearray, memoryview and numpy arrays are taken without a copy)"""
    a = blob if isinstance(blob, np.ndarray) else np.frombuffer(blob, dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _struct_dict(st):
    """a ctypes struct as a dict of its fields"""
    return {k: getattr(st, k) for k, _ in st._fields_}


def _config_dict(c):
    """fskhip_config -> FSKConfig dict (every field, the reference's names)"""
    return dict(sampleRate=c.sampleRate, baudRate=c.baudRate, markFrequency=c.markFrequency, spaceFrequency=c.spaceFrequency,
                preamblePattern=list(c.preamblePattern)[:c.preambleLen], sfdPattern=list(c.sfdPattern)[:c.sfdLen],
                startBits=c.startBits, stopBits=c.stopBits, parity=_PARITY_NAME[c.parity], syncThreshold=c.syncThreshold,
                agcEnabled=bool(c.agcEnabled), preFilterBandwidth=c.preFilterBandwidth, adaptiveThreshold=bool(c.adaptiveThreshold))


def snapshot_info(blob):
    """fskhip_snapshot_info_get: what a stream snapshot holds (validated on the host, no device needed)"""
    b = _blob(blob)
    info = _lib.SnapshotInfo()
    _lib.check(_lib.lib().fskhip_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


def snapshot_stream_config(blob, i):
    """fskhip_snapshot_stream_config: the FSKConfig dict record i of a snapshot ran under"""
    b = _blob(blob)
    c = Config()
    _lib.check(_lib.lib().fskhip_snapshot_stream_config(b.ctypes.data, b.nbytes, int(i), C.byref(c)))
    return _config_dict(c)


def snapshot_concat(blobs):
    """fskhip_snapshot_concat: one snapshot holding the records of `blobs` in order.  They must be images of engines that
    could have been ONE engine (shards of a sharded batch, created together and fed the same calls); refused otherwise."""
    bs = [_blob(b) for b in blobs]
    L = _lib.lib()
    ptrs = (C.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    sizes = (C.c_size_t * len(bs))(*[b.nbytes for b in bs])
    need = C.c_size_t(0)
    rc = L.fskhip_snapshot_concat(ptrs, sizes, len(bs), None, 0, C.byref(need))
    if rc != _lib.E_OVERFLOW:
        _lib.check(rc)
    out = np.zeros(need.value, np.uint8)
    _lib.check(L.fskhip_snapshot_concat(ptrs, sizes, len(bs), out.ctypes.data, out.nbytes, C.byref(need)))
    return out


def _snapshot_plan(blob, stream_map, configs, range_error=True):
    """What every from_snapshot starts with: (snapshot_info(blob), the map as an int64 array, the configs).  stream_map None
    is every record in order.  configs None: read out of the snapshot -- the shared one, or record by record through the
    map, where a -1 slot has none to take.  An entry past the records raises ValueError here if range_error; else it is left
    to the library's refusal."""
    info = snapshot_info(blob)
    n = info["n_streams"]
    m = np.arange(n, dtype=np.int64) if stream_map is None else np.asarray(stream_map, dtype=np.int64).reshape(-1)
    if configs is None:
        if not info["per_stream_configs"]:
            configs = snapshot_stream_config(blob, 0)
        else:
            if (m < 0).any():
                raise ValueError("a -1 slot needs an explicit config: the snapshot has per-stream configs")
            if range_error and (m >= n).any():
                raise ValueError("stream map entry out of range (%d records)" % n)
            known = {}
            configs = [known.setdefault(v, snapshot_stream_config(blob, v)) for v in m.tolist()]
    return info, m, configs


# capture formats and layouts by name (include/fskhip.h: FSKHIP_SAMPLES_* / FSKHIP_LAYOUT_*)
SAMPLE_FORMATS = {"f32": _lib.SAMPLES_F32, "s16": _lib.SAMPLES_S16, "mulaw": _lib.SAMPLES_MULAW, "alaw": _lib.SAMPLES_ALAW}
SAMPLE_LAYOUTS = {"stream": _lib.LAYOUT_STREAM_MAJOR, "sample": _lib.LAYOUT_SAMPLE_MAJOR}
_FORMAT_DTYPE = {_lib.SAMPLES_F32: np.float32, _lib.SAMPLES_S16: np.int16, _lib.SAMPLES_MULAW: np.uint8, _lib.SAMPLES_ALAW: np.uint8}


def _sample_codes(fmt, layout, numbers_as_they_are=False):
    """(format, layout) as the library's numbers, from names (SAMPLE_FORMATS / SAMPLE_LAYOUTS, any case) or numbers.
    numbers_as_they_are: a number that is no format or layout is passed on, for the library to refuse."""
    code = SAMPLE_FORMATS.get(fmt.lower()) if isinstance(fmt, str) else int(fmt)
    lay = SAMPLE_LAYOUTS.get(layout.lower()) if isinstance(layout, str) else int(layout)
    if code not in _FORMAT_DTYPE and not (numbers_as_they_are and code is not None):
        raise ValueError("unknown sample format %r (one of %s)" % (fmt, ", ".join(SAMPLE_FORMATS)))
    if lay not in SAMPLE_LAYOUTS.values() and not (numbers_as_they_are and lay is not None):
        raise ValueError("unknown layout %r (one of %s)" % (layout, ", ".join(SAMPLE_LAYOUTS)))
    return code, lay


def _row_pitch(a):
    """the pitch in elements of a 2-D array whose rows are contiguous and lie at one constant pitch of whole elements, at least a
    row apart (a block of rows or of columns of a wider array is one); None for any other"""
    isz = a.dtype.itemsize
    rows, cols = a.shape
    if not (cols <= 1 or a.strides[1] == isz) or not (rows <= 1 or (a.strides[0] % isz == 0 and a.strides[0] >= cols * isz)):
        return None
    return max(a.strides[0] // isz if rows > 1 else cols, cols, 1)


def sample_args(samples, fmt=None, layout="stream"):
    """What fskhip_demodulate_host_fmt takes for a numpy array of capture samples: (array, format, layout, streams, samples per
    stream, pitch in elements).  fmt None: by the dtype -- float32 is "f32", int16 "s16"; uint8 needs "mulaw" or "alaw" said.
    layout "stream": the array is [S, N]; "sample": [N, S], interleaved frames.  A view whose rows are a block of a wider array
    (a shard of it) is taken as it is, with the wider array's pitch; anything else that is not contiguous is copied."""
    a = np.asarray(samples)
    if fmt is None:
        if a.dtype == np.float32:
            fmt = _lib.SAMPLES_F32
        elif a.dtype == np.int16:
            fmt = _lib.SAMPLES_S16
        elif a.dtype == np.uint8:
            raise ValueError("uint8 samples need fmt='mulaw' or fmt='alaw'")
        else:
            raise ValueError("no sample format for dtype %s: float32, int16 or uint8 (G.711)" % a.dtype)
    code, lay = _sample_codes(fmt, layout)
    if a.dtype != _FORMAT_DTYPE[code]:
        raise ValueError("format %r takes %s samples, got %s" % (fmt, np.dtype(_FORMAT_DTYPE[code]).name, a.dtype))
    if a.ndim == 1:
        a = a.reshape(1, -1) if lay == _lib.LAYOUT_STREAM_MAJOR else a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError("samples must be a 2-D array")
    if _row_pitch(a) is None:
        a = np.ascontiguousarray(a)
    S, N = a.shape if lay == _lib.LAYOUT_STREAM_MAJOR else a.shape[::-1]
    return a, code, lay, S, N, _row_pitch(a)


def ingest_device(d_src, fmt, layout, n_streams, n_per_stream, src_pitch, d_dst, dst_pitch, stream=None):
    """fskhip_ingest_device: device pointers (ints); widens capture samples into float32 [n_streams][dst_pitch] on the current
    device, asynchronously on `stream` (a hipStream_t handle or None)."""
    _lib.check(_lib.lib().fskhip_ingest_device(d_src, *_sample_codes(fmt, layout, True), n_streams, n_per_stream, src_pitch,
                                               d_dst, dst_pitch, stream))


def egress_device(d_src, src_pitch, d_lens, n_streams, n_per_stream, fmt, layout, d_dst, dst_pitch, stream=None):
    """fskhip_egress_device: device pointers (ints); narrows float32 [n_streams][src_pitch] into samples of `fmt` in `layout` on the
    current device, asynchronously on `stream` (a hipStream_t handle or None).  d_lens (or None): per-stream lengths; a stream is
    the format's silence from its length on."""
    _lib.check(_lib.lib().fskhip_egress_device(d_src, src_pitch, d_lens, n_streams, n_per_stream, *_sample_codes(fmt, layout, True),
                                               d_dst, dst_pitch, stream))


def payload_args(payloads):
    """What the modulate calls take for a list of bytes-like payloads: (uint8 [S, pitch] array, uint32 lengths, pitch)"""
    lens = np.array([len(p) for p in payloads], dtype=np.uint32)
    ppitch = max(1, int(lens.max())) if len(lens) else 1
    pay = np.zeros((len(payloads), ppitch), dtype=np.uint8)
    for s, p in enumerate(payloads):
        if len(p):
            pay[s, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
    return pay, lens, ppitch


def samples_out(fmt, layout, n_streams, n_per_stream, out=None):
    """The array FSKEngine.modulate_samples writes: (array, format, layout, pitch in elements).  out None: a new one of the format's
    dtype (SAMPLE_FORMATS), [S, n] (layout "stream") or [n, S] (layout "sample").  Otherwise `out` itself, which must have that
    dtype and shape and unit stride along its rows; its rows may be a block of a wider array (a shard's column block of
    interleaved frames): the wider array's pitch is passed on and nothing is copied."""
    code, lay = _sample_codes(fmt, layout)
    shape = (n_streams, n_per_stream) if lay == _lib.LAYOUT_STREAM_MAJOR else (n_per_stream, n_streams)
    if out is None:
        out = np.zeros(shape, _FORMAT_DTYPE[code])
    if not isinstance(out, np.ndarray) or out.dtype != _FORMAT_DTYPE[code] or out.shape != shape or not out.flags.writeable:
        raise ValueError("out must be a writeable %s array of shape %r" % (np.dtype(_FORMAT_DTYPE[code]).name, shape))
    if not out.size:              # (no elements -- a rate converter's call that writes nothing: no strides to speak of, the rows are packed)
        return out, code, lay, max(shape[1], 1)
    if _row_pitch(out) is None:
        raise ValueError("out must have contiguous rows at a constant pitch")
    return out, code, lay, _row_pitch(out)


# Called with (n_streams, precision) by every new FSKEngine; returns a dict of fskhip_set_option() names -> values to apply on
# top of the `options` argument, or None.  The package sets nothing here and reads no environment variable; the test suite
# (tests/conftest.py) and the measurement tools (tools/envopts.py) install a hook that maps their FSKHIP_* variables.
option_hook = None


class FSKEngine:
    """S FSKCore instances on one GPU.

    configs: one FSKConfig dict (shared) or a list of S dicts that differ only in
    markFrequency / spaceFrequency / preFilterBandwidth (BASELINE config #4).
    options: tuning / test switches by name (include/fskhip.h, fskhip_set_option); none changes a result.
    """

    def __init__(self, n_streams, configs=None, device=0, precision=PRECISION_F32, options=None):
        L = _lib.lib()
        if isinstance(configs, (list, tuple)):
            if len(configs) != n_streams:
                raise ValueError("need one config per stream")
            made = [make_config(c) for c in configs]
            self._configs, self._config_arg = [dict(c or {}) for c in configs], None
            arr = (Config * n_streams)(*[m[0] for m in made])
            self.config = made[0][1]
            n_cfgs = n_streams
        else:
            c, self.config = make_config(configs)
            self._configs, self._config_arg = None, dict(configs or {})
            arr = (Config * 1)(c)
            n_cfgs = 1
        h = C.c_void_p()
        _lib.check(L.fskhip_create(arr, n_cfgs, n_streams, device, precision, C.byref(h)))
        self._h = h
        self._L = L
        self.n_streams = n_streams
        self.device = device
        self.precision = precision
        opts = dict(options or {})
        if option_hook is not None:
            opts.update(option_hook(n_streams, precision) or {})
        try:
            for k, v in opts.items():
                self.set_option(k, v)
        except Exception:
            self.close()
            raise

    def set_option(self, name, value):
        """fskhip_set_option (include/fskhip.h): before the first demodulate call"""
        _lib.check(self._L.fskhip_set_option(self._h, str(name).encode(), str(value).encode()))

    def close(self):
        if getattr(self, "_h", None):
            for ptr, _cap in self.__dict__.pop("_at_scratch", {}).values():
                self._L.fskhip_device_free(self._h, ptr)
            self._L.fskhip_destroy(self._h)
            self._h = None

    def carry_over_from(self, old):
        """what FSKCore.configure() leaves in place on a configured instance: silence threshold, debug counters"""
        _lib.check(self._L.fskhip_carry_over(self._h, old._h))

    def remap_from(self, src, stream_map):
        """fskhip_remap_streams: stream i of this (new, not yet demodulated) engine continues stream stream_map[i] of `src`
        as if that FSKCore had been moved, or starts afresh where stream_map[i] is -1.  `src` is left as it is."""
        m = np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        _lib.check(self._L.fskhip_remap_streams(self._h, src._h, m.ctypes.data, len(m)))

    def remapped(self, stream_map, configs=None, options=None):
        """A new engine of len(stream_map) streams whose stream i continues stream stream_map[i] of this one (-1: a new
        FSKCore).  Its configs are taken from this engine by the map unless given; a -1 slot needs an explicit config when this
        engine has per-stream configs.  `options` are the new engine's own (fskhip_set_option)."""
        m = [int(v) for v in np.asarray(stream_map, dtype=np.int64).reshape(-1)]
        if configs is None:
            if self._configs is None:
                configs = self._config_arg
            else:
                if any(v < 0 for v in m):
                    raise ValueError("a -1 slot needs an explicit config: this engine has per-stream configs")
                if any(v >= self.n_streams for v in m):
                    raise ValueError("stream map entry out of range (%d streams)" % self.n_streams)
                configs = [self._configs[v] for v in m]
        eng = FSKEngine(len(m), configs, device=self.device, precision=self.precision, options=options)
        try:
            eng.remap_from(self, m)
        except Exception:
            eng.close()
            raise
        return eng

    # ---- stream snapshots (include/fskhip.h): a portable image of streams, restored under the remap's contract ----------
    def snapshot(self, streams=None, out=None):
        """fskhip_snapshot_streams: a numpy uint8 array holding streams `streams` of this engine (None: all, in order; a
        stream may be named more than once) -- plain bytes, fit for a file.  The engine is read only and stays usable.
        `out`: a uint8 array to write into (pinned_empty(...) makes the copy faster); a view of it is returned."""
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int64).reshape(-1)
        n = self.n_streams if sel is None else len(sel)
        need = int(self._L.fskhip_snapshot_bytes(self._h, n))
        buf = np.zeros(need, np.uint8) if out is None else out
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array")
        w = C.c_size_t(0)
        _lib.check(self._L.fskhip_snapshot_streams(self._h, None if sel is None else sel.ctypes.data, n, buf.ctypes.data, buf.nbytes, C.byref(w)))
        return buf.reshape(-1)[:w.value]

    def restore_from(self, blob, stream_map):
        """fskhip_restore_streams: stream i of this (new, not yet demodulated) engine continues RECORD stream_map[i] of the
        snapshot `blob` as if that FSKCore had been moved here, or starts afresh where stream_map[i] is -1."""
        b = _blob(blob)
        m = np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        _lib.check(self._L.fskhip_restore_streams(self._h, b.ctypes.data, b.nbytes, m.ctypes.data, len(m)))

    @classmethod
    def from_snapshot(cls, blob, stream_map=None, configs=None, device=0, options=None):
        """A new engine on `device` that continues the records of a snapshot: stream i continues record stream_map[i] (-1: a
        new FSKCore; None: every record, in order).  Precision and configs are read out of the snapshot unless `configs` is
        given; a -1 slot needs an explicit config when the snapshot's configs are per stream."""
        b = _blob(blob)
        info, m, configs = _snapshot_plan(b, stream_map, configs)
        eng = cls(len(m), configs, device=device, precision=info["precision"], options=options)
        try:
            eng.restore_from(b, m)
        except Exception:
            eng.close()
            raise
        return eng

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- demodulateData (fsk.ts:190-222) -------------------------------------------------------
    def max_bytes(self, n_per_stream):
        """Upper bound on bytes one call can produce per stream (fskhip_max_bytes: size out_pitch with it)."""
        return int(self._L.fskhip_max_bytes(self._h, int(n_per_stream)))

    def last_kernel(self):
        """Name of the kernel the last demodulate_device call launched for its whole tiles (fskhip_last_kernel)."""
        return (self._L.fskhip_last_kernel(self._h) or b"").decode()

    def blk_lanes(self):
        """Streams per workgroup of the four-wave kernel for this engine (fskhip_blk_lanes): 64, 32, 16, 8, or 0."""
        return int(self._L.fskhip_blk_lanes(self._h))

    def demodulate_data(self, samples, writeback_agc=False, out_pitch=None):
        """samples: float32 [S, N] (host).  Returns (list of bytes per stream, eod counts ndarray).

        With writeback_agc=True `samples` is overwritten with the AGC-scaled samples, the side
        effect the reference has on its input buffer (fsk.ts:55, 201).
        """
        x = samples if (writeback_agc and isinstance(samples, np.ndarray) and samples.dtype == np.float32
                        and samples.flags.c_contiguous) else np.ascontiguousarray(samples, dtype=np.float32)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        S, N = x.shape
        if S != self.n_streams:
            raise ValueError("expected %d streams, got %d" % (self.n_streams, S))
        pitch = out_pitch or self.max_bytes(N)
        out = np.zeros((S, pitch), dtype=np.uint8)
        counts = np.zeros(S, dtype=np.uint32)
        eod = np.zeros(S, dtype=np.uint32)
        flags = DEMOD_WRITEBACK_AGC if writeback_agc else 0
        _lib.check(self._L.fskhip_demodulate_host(
            self._h, x.ctypes.data, N, x.strides[0] // 4 if N else max(N, 1), out.ctypes.data, pitch,
            counts.ctypes.data, eod.ctypes.data, flags))
        if writeback_agc and x is not samples:
            np.copyto(samples, x.reshape(samples.shape))
        return [out[s, :counts[s]].tobytes() for s in range(S)], eod

    def demodulate_samples(self, samples, fmt=None, layout="stream", out_pitch=None):
        """demodulate_data for capture samples as they arrive (fskhip_demodulate_host_fmt): int16 PCM, G.711 bytes (uint8 with
        fmt="mulaw" / "alaw") or float32, [S, N] (layout="stream") or interleaved frames [N, S] (layout="sample").  The narrow
        samples cross PCIe and are widened on the device.  Returns what demodulate_data returns."""
        x, code, lay, S, N, pitch = sample_args(samples, fmt, layout)
        if S != self.n_streams:
            raise ValueError("expected %d streams, got %d" % (self.n_streams, S))
        opitch = out_pitch or self.max_bytes(N)
        out = np.zeros((S, opitch), dtype=np.uint8)
        counts = np.zeros(S, dtype=np.uint32)
        eod = np.zeros(S, dtype=np.uint32)
        _lib.check(self._L.fskhip_demodulate_host_fmt(self._h, x.ctypes.data, code, lay, N, pitch, out.ctypes.data, opitch,
                                                      counts.ctypes.data, eod.ctypes.data, 0))
        return [out[s, :counts[s]].tobytes() for s in range(S)], eod

    def demodulate_samples_at(self, samples, fmt, layout, upsampler, out_pitch=None, any_length=False):
        """demodulate_samples for capture samples at a lower rate (8 kHz trunk audio in front of a 48 kHz engine): the narrow
        samples cross PCIe as they are, `upsampler` (filters.Upsampler, on this engine's device, its history carried from call to
        call) widens and interpolates them into a device tile, and demodulate_device runs on that tile.  `upsampler` may also be a
        filters.CaptureConverter (44.1 kHz captures: 160 / 147); the samples per stream must then be a multiple of its `down`.
        any_length=True (a CaptureConverter only) takes any number of samples per stream, from the handle's position -- a capture
        file of 44.1 kHz audio cut as it comes: process_any_device, then demodulate_device on the out_count_any(n) engine samples
        it wrote; where that is none, the handle still takes its samples, nothing is demodulated and the returns are empty.  A
        multiple of `down` from position 0 runs the calls it runs without the flag.
        Returns what demodulate_data returns."""
        from .filters import CaptureConverter
        x, code, lay, S, N, _ = sample_args(samples, fmt, layout)
        if S != self.n_streams or upsampler.n_streams != S:
            raise ValueError("expected %d streams, got %d (upsampler: %d)" % (self.n_streams, S, upsampler.n_streams))
        if upsampler.device != self.device:
            raise ValueError("the upsampler is on device %d, the engine on %d" % (upsampler.device, self.device))
        eod = np.zeros(S, dtype=np.uint32)
        if any_length and not isinstance(upsampler, CaptureConverter):
            raise TypeError("upsampler is a %s: calls of any length go through a filters.CaptureConverter" % type(upsampler).__name__)
        if N == 0:
            return [b""] * S, eod
        x = np.ascontiguousarray(x)
        any_length = any_length and (N % upsampler.down != 0 or upsampler.position != 0)
        if any_length:
            n = upsampler.out_count_any(N)
        elif isinstance(upsampler, CaptureConverter):
            if N % upsampler.down:
                raise ValueError("%d samples per stream are not a multiple of the converter's down factor %d" % (N, upsampler.down))
            n = upsampler.out_count(N)
        else:
            n = N * upsampler.factor
        tpitch = max((n + 3) & ~3, 4)      # (a call that completes no engine sample still hands the converter a tile)
        opitch = out_pitch or self.max_bytes(n)
        out = np.zeros((S, opitch), dtype=np.uint8)
        counts = np.zeros(S, dtype=np.uint32)
        d_src, d_tile, d_out, d_counts, d_eod = (self._scratch(k, b) for k, b in (("narrow", x.nbytes), ("tile", 4 * S * tpitch), ("bytes", out.nbytes),
                                                                                  ("counts", 4 * S), ("eod", 4 * S)))
        self.h2d(d_src, x)
        if any_length:
            upsampler.process_any_device(d_src, code, lay, N, x.shape[1], d_tile, tpitch)
            if n == 0:      # the handle has taken its samples; they completed no engine sample
                self.synchronize()
                return [b""] * S, eod
        else:
            upsampler.process_device(d_src, code, lay, N, x.shape[1], d_tile, tpitch)
        self.demodulate_device(d_tile, n, tpitch, d_out, opitch, d_counts, d_eod)
        self.synchronize()
        for a, d in ((out, d_out), (counts, d_counts), (eod, d_eod)):
            self.d2h(a, d)
        return [out[s, :counts[s]].tobytes() for s in range(S)], eod

    def _scratch(self, name, nbytes):
        """a device buffer of the *_samples_at calls, kept with the engine and only ever grown (freed by close())"""
        slots = self.__dict__.setdefault("_at_scratch", {})
        ptr, cap = slots.get(name, (None, 0))
        if cap < nbytes:
            if ptr:
                self.synchronize()
                self.device_free(ptr)
                slots.pop(name)
            cap = max(16, int(nbytes))
            ptr = self.device_malloc(cap)
            slots[name] = (ptr, cap)
        return ptr

    def demodulate_device(self, d_samples, n_per_stream, pitch, d_out, out_pitch, d_counts, d_eod=None,
                          flags=0, stream=None):
        """Device-pointer form (ints): asynchronous on `stream` (a hipStream_t handle or None)."""
        _lib.check(self._L.fskhip_demodulate_device(self._h, d_samples, n_per_stream, pitch, d_out, out_pitch,
                                                    d_counts, d_eod, flags, stream))

    # ---- modulateData (fsk.ts:377-424) ---------------------------------------------------------
    def modulated_length(self, n_bytes):
        return int(self._L.fskhip_modulated_length(self._h, n_bytes))

    def modulate_data(self, payloads):
        """payloads: list of S bytes-like.  Returns list of float32 arrays (one signal per stream)."""
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        S = self.n_streams
        pay, lens, ppitch = payload_args(payloads)
        opitch = max(4, self.modulated_length(int(lens.max())))
        out = np.zeros((S, opitch), dtype=np.float32)
        out_lens = np.zeros(S, dtype=np.uint32)
        _lib.check(self._L.fskhip_modulate_host(self._h, pay.ctypes.data, lens.ctypes.data, ppitch, out.ctypes.data,
                                                opitch, out_lens.ctypes.data))
        return [out[s, :out_lens[s]].copy() for s in range(S)]

    def modulate_samples(self, payloads, fmt, layout="stream", n_per_stream=None, out=None):
        """modulate_data into playback samples as a trunk or a sound card takes them (fskhip_modulate_host_fmt): fmt "s16", "mulaw",
        "alaw" or "f32", [S, n] (layout="stream") or interleaved frames [n, S] (layout="sample"); quantised on the device, so the
        narrow samples are what crosses PCIe.  n_per_stream None: the longest signal's length.  Returns (samples, lens): stream s
        is the format's silence from lens[s] on.  `out`: the array to write into (samples_out)."""
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        S = self.n_streams
        pay, lens, ppitch = payload_args(payloads)
        n = self.modulated_length(int(lens.max())) if n_per_stream is None else int(n_per_stream)
        out, code, lay, pitch = samples_out(fmt, layout, S, n, out)
        out_lens = np.zeros(S, dtype=np.uint32)
        _lib.check(self._L.fskhip_modulate_host_fmt(self._h, pay.ctypes.data, lens.ctypes.data, ppitch, code, lay, out.ctypes.data, n, pitch,
                                                    out_lens.ctypes.data))
        return out, out_lens

    def modulate_samples_at(self, payloads, fmt, layout, downsampler, n_per_stream=None, any_length=False):
        """modulate_samples at a lower rate (a 48 kHz engine in front of an 8 kHz trunk): modulate_device writes the float tile,
        `downsampler` (filters.Downsampler, on this engine's device) decimates it with every stream's samples behind its own
        signal read as zeros, and one narrow copy comes back.  n_per_stream: low rate samples per stream (None: what the longest
        signal and the filter's ringing behind it take).  Returns (samples, lens): [S, n] or frames [n, S], and each stream's low
        rate length ceil((len + n_taps - 1) / factor), from where on it is the format's silence.  `downsampler` may also be a
        filters.PlaybackConverter (towards 44.1 kHz: 147 / 160): n_per_stream then counts its output samples and the lengths are
        its out_length of each stream's signal, capped at n.  any_length=True (a PlaybackConverter only) writes exactly
        n_per_stream samples from the handle's position, whatever both are, through process_any_device on the
        in_count_any(n_per_stream) engine samples that takes, and the handle moves on by those (without it the handle converts
        whole periods, ceil(n / up) of them, and stays at its position); an n_per_stream the handle cannot write from its position
        (only where up > down) is a ValueError in the processor's words.  The lengths are then the outputs of the call that the
        stream's signal and the ringing behind it reach.  A multiple of `up` from position 0 runs the calls it runs without the
        flag."""
        from .filters import PlaybackConverter
        if any_length and not isinstance(downsampler, PlaybackConverter):
            raise TypeError("downsampler is a %s: calls of any length go through a filters.PlaybackConverter" % type(downsampler).__name__)
        if isinstance(downsampler, PlaybackConverter):
            return self._modulate_samples_converted(payloads, fmt, layout, downsampler, n_per_stream, any_length)
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        S, L = self.n_streams, downsampler.factor
        if downsampler.n_streams != S or downsampler.device != self.device:
            raise ValueError("the downsampler must have this engine's %d streams and device %d" % (S, self.device))
        pay, lens, ppitch = payload_args(payloads)
        n = downsampler.low_rate_length(self.modulated_length(int(lens.max()))) if n_per_stream is None else int(n_per_stream)
        out, code, lay, pitch = samples_out(fmt, layout, S, n)
        out_lens = np.zeros(S, dtype=np.uint32)
        if n == 0:
            return out, out_lens
        tpitch = (n * L + 3) & ~3
        d_pay, d_plens, d_tile, d_lens, d_dst = (self._scratch(k, b) for k, b in (("payloads", pay.nbytes), ("payload_lens", lens.nbytes), ("tile", 4 * S * tpitch),
                                                                                  ("counts", 4 * S), ("narrow", out.nbytes)))
        self.h2d(d_pay, pay)
        self.h2d(d_plens, lens)
        self.modulate_device(d_pay, d_plens, ppitch, d_tile, tpitch, d_lens)
        self.synchronize()
        self.d2h(out_lens, d_lens)
        if int(out_lens.max()) > n * L:           # refused before the decimator runs: its history stays as it was
            s = int(np.argmax(out_lens > n * L))
            raise FskHipError(_lib.E_OVERFLOW, "stream %d needs %d samples, slab holds %d" % (s, out_lens[s], n * L))
        downsampler.process_device(d_tile, n * L, tpitch, d_lens, d_dst, code, lay, pitch)
        self.synchronize()
        self.d2h(out, d_dst)
        return out, np.minimum((out_lens.astype(np.int64) + len(downsampler.taps) - 1 + L - 1) // L, n).astype(np.uint32)

    def _modulate_samples_converted(self, payloads, fmt, layout, converter, n_per_stream, any_length=False):
        """modulate_samples_at through a filters.PlaybackConverter (a 48 kHz engine in front of a 44.1 kHz sound card): the float
        tile is padded to a whole number of the converter's periods, so the call writes ceil(n / up) * up samples per stream on
        the device and the first n come back.  The lengths are the converter's out_length of each stream's signal, capped at n.
        any_length: the call starts at the handle's position pos and writes exactly n through process_any_device on
        in_count_any(n) engine samples (a multiple of `up` from position 0: the padded call above, which is the same call); n
        defaults to the outputs from pos that the longest signal and the ringing behind it reach, and the lengths are each
        stream's count of those, capped at n."""
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        S = self.n_streams
        if converter.n_streams != S or converter.device != self.device:
            raise ValueError("the converter must have this engine's %d streams and device %d" % (S, self.device))
        pay, lens, ppitch = payload_args(payloads)
        pos = converter.position if any_length else 0
        first = -(-pos * converter.up // converter.down)      # the first output of the period grid that a call from pos writes

        def reach(v):      # outputs of a call from pos that a signal of v samples and its ringing reach (pos 0: out_length(v))
            return max(converter.out_length(pos + int(v)) - first, 0) if v else 0
        n = reach(self.modulated_length(int(lens.max()))) if n_per_stream is None else int(n_per_stream)
        out_lens = np.zeros(S, dtype=np.uint32)
        if n == 0:
            return samples_out(fmt, layout, S, 0)[0], out_lens
        any_length = any_length and (n % converter.up != 0 or pos != 0)
        if any_length:      # exactly n from the handle's position
            n_in, n_dev = converter.in_count_any(n), n
            above = converter.out_count_any(n_in)
            if above != n:
                raise ValueError("the playback handle at position %d cannot write n_out %d: %d engine samples give %d, %d give %d"
                                 % (pos, n, n_in - 1, converter.out_count_any(n_in - 1), n_in, above))
        else:
            periods = -(-n // converter.up)
            n_in, n_dev = periods * converter.down, periods * converter.up
        full, code, lay, pitch = samples_out(fmt, layout, S, n_dev)
        tpitch = (n_in + 3) & ~3
        d_pay, d_plens, d_tile, d_lens, d_dst = (self._scratch(k, b) for k, b in (("payloads", pay.nbytes), ("payload_lens", lens.nbytes), ("tile", 4 * S * tpitch),
                                                                                  ("counts", 4 * S), ("narrow", full.nbytes)))
        self.h2d(d_pay, pay)
        self.h2d(d_plens, lens)
        self.modulate_device(d_pay, d_plens, ppitch, d_tile, tpitch, d_lens)
        self.synchronize()
        self.d2h(out_lens, d_lens)
        if int(out_lens.max()) > n_in:            # refused before the converter runs: its history stays as it was
            s = int(np.argmax(out_lens > n_in))
            raise FskHipError(_lib.E_OVERFLOW, "stream %d needs %d samples, slab holds %d" % (s, out_lens[s], n_in))
        if any_length:
            converter.process_any_device(d_tile, n_in, tpitch, d_lens, d_dst, code, lay, pitch)
        else:
            converter.process_device(d_tile, n_in, tpitch, d_lens, d_dst, code, lay, pitch)
        self.synchronize()
        self.d2h(full, d_dst)
        out = np.ascontiguousarray(full[:, :n] if lay == _lib.LAYOUT_STREAM_MAJOR else full[:n])
        # (output j of the period grid is the call's j - first; a signal of v samples from position pos reaches the outputs up to
        # out_length(pos + v) - 1 of the grid)
        return out, np.array([min(reach(v), n) for v in out_lens], dtype=np.uint32)

    def modulate_device(self, d_payloads, d_lens, payload_pitch, d_out, out_pitch, d_out_lens, stream=None):
        _lib.check(self._L.fskhip_modulate_device(self._h, d_payloads, d_lens, payload_pitch, d_out, out_pitch,
                                                  d_out_lens, stream))

    # ---- reset / getStatus ---------------------------------------------------------------------
    def reset(self, stream=-1):
        _lib.check(self._L.fskhip_reset(self._h, stream))

    def get_status(self, stream=0):
        st = Status()
        _lib.check(self._L.fskhip_get_status(self._h, stream, C.byref(st)))
        return _status_dict(st)

    def faults(self):
        """uint8[S]: 1 = the stream's filter state is no longer finite (fskhip_get_faults): it absorbed a NaN / Inf sample -- the
        reference's instance is dead from there on too, and the engine does what it does -- or, fp32 engines only, a sample beyond
        their range (~1e19)."""
        out = np.zeros(self.n_streams, np.uint8)
        n = C.c_uint32(0)
        _lib.check(self._L.fskhip_get_faults(self._h, out.ctypes.data, C.byref(n)))
        assert int(out.sum()) == n.value
        return out

    def fault(self, stream=0):
        return bool(self.faults()[stream])

    # ---- opt-in signal-quality estimates (include/fskhip.h; the reference's getSignalQuality() returns zeros) -------
    def enable_signal_quality(self, on=True):
        _lib.check(self._L.fskhip_enable_signal_quality(self._h, 1 if on else 0))

    def get_signal_quality(self, stream=0):
        q = _lib.SignalQuality()
        _lib.check(self._L.fskhip_get_signal_quality(self._h, stream, C.byref(q)))
        return {k: getattr(q, k) for k, _ in _lib.SignalQuality._fields_}

    def demod_supported(self):
        return bool(self._L.fskhip_demod_supported(self._h))

    # ---- intermediate capture (parity tests) -----------------------------------------------------
    def trace_enable(self, stream, capacity):
        _lib.check(self._L.fskhip_trace_enable(self._h, stream, capacity))
        self._trace_cap = capacity

    def trace_read(self):
        cap = self._trace_cap
        amp = np.zeros(cap, np.float64)
        post = np.zeros(cap, np.float64)
        bit = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        _lib.check(self._L.fskhip_trace_read(self._h, amp.ctypes.data, post.ctypes.data, bit.ctypes.data, cap,
                                             C.byref(n)))
        pre = np.zeros(2 * cap, np.float64)
        npre = C.c_size_t(0)
        _lib.check(self._L.fskhip_trace_read_pre(self._h, pre.ctypes.data, 2 * cap, C.byref(npre)))
        return {"amp": amp[:n.value], "post_out": post[:n.value], "bit": bit[:n.value], "pre_out": pre[:min(npre.value, 2 * cap)]}

    # ---- measurement tooling -------------------------------------------------------------------
    def synth_device(self, d_out, n_per_stream, pitch, payload_len, seed, lead_max, amp_lo, amp_hi, stream=None):
        _lib.check(self._L.fskhip_synth_device(self._h, d_out, n_per_stream, pitch, payload_len, seed, lead_max,
                                               amp_lo, amp_hi, stream))

    def add_awgn_device(self, d_buf, n_per_stream, pitch, snr_db, seed, stream=None):
        _lib.check(self._L.fskhip_add_awgn_device(self._h, d_buf, n_per_stream, pitch, snr_db, seed, stream))

    def probe_read_device(self, d_buf, n_per_stream, pitch, stream=None):
        _lib.check(self._L.fskhip_probe_read_device(self._h, d_buf, n_per_stream, pitch, stream))

    def synth_payload(self, seed, stream, frame, payload_len):
        f = self._L.fskhip_synth_payload_byte
        return bytes(f(seed, stream, frame, i) for i in range(payload_len))

    def synth_stream_params(self, seed, stream, lead_max, amp_lo, amp_hi):
        lead, amp = C.c_uint32(), C.c_double()
        self._L.fskhip_synth_stream_params(seed, stream, lead_max, amp_lo, amp_hi, C.byref(lead), C.byref(amp))
        return lead.value, amp.value

    def device_malloc(self, nbytes):
        p = C.c_void_p()
        _lib.check(self._L.fskhip_device_malloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, ptr):
        _lib.check(self._L.fskhip_device_free(self._h, ptr))

    def h2d(self, d_dst, arr):
        a = np.ascontiguousarray(arr)
        _lib.check(self._L.fskhip_memcpy_h2d(self._h, d_dst, a.ctypes.data, a.nbytes))

    def d2h(self, arr, d_src):
        assert arr.flags.c_contiguous
        _lib.check(self._L.fskhip_memcpy_d2h(self._h, arr.ctypes.data, d_src, arr.nbytes))

    def synchronize(self):
        _lib.check(self._L.fskhip_synchronize(self._h))

    def debug_state(self, stream):
        """(real words, integer words) of one stream's carried state, fsk_params.h order (diagnostics)"""
        r, i = (C.c_double * 128)(), (C.c_uint32 * 128)()
        nr, ni = C.c_uint32(), C.c_uint32()
        _lib.check(self._L.fskhip_debug_state(self._h, stream, r, 128, i, 128, C.byref(nr), C.byref(ni)))
        return list(r[:nr.value]), list(i[:ni.value])

    def clock_probe_begin(self, spin_ms):
        """start the shader-clock probe (include/fskhip.h); launch the work to observe behind it on other streams"""
        _lib.check(self._L.fskhip_clock_probe_begin(self._h, float(spin_ms)))

    def clock_probe_end(self):
        """-> (shader clock in GHz, milliseconds the probe covered)"""
        ghz, ms = C.c_double(), C.c_double()
        _lib.check(self._L.fskhip_clock_probe_end(self._h, C.byref(ghz), C.byref(ms)))
        return ghz.value, ms.value

    def timing_begin(self):
        _lib.check(self._L.fskhip_timing_begin(self._h))

    def timing_end(self):
        n, ms = C.c_uint32(), C.c_double()
        _lib.check(self._L.fskhip_timing_end(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value
