"""The streaming contract either side of FSKCore, above the C ABI (include/fskhip_next.h):

* `ChunkedModulator` -- src/webaudio/chunked-modulator.ts, same method names, over any object with the
  `modulateData(bytes)` of `FSKCore` (the GPU modulator);
* `FSKProcessorBatch` -- S instances of src/webaudio/processors/fsk-processor.ts on one GPU: `process()` once per
  quantum for all streams (RX byte rings and pending modulations stay on the device), `modulate`, `demodulate`,
  `reset`, `status`; and the batch's lifecycle -- `remapped`, `snapshot`, `from_snapshot` -- which carries the rings and
  pending modulations along with the engine's streams.
"""
import ctypes as C

import collections

import numpy as np

from . import _lib
from ._lib import PROC_CLEAR_RX_ON_TX_COMPLETE, PROC_GRAPH, PROC_RATECVT_PAIR  # noqa: F401
from .engine import FSKEngine, _blob, _struct_dict, _sample_codes, sample_args, samples_out


class ChunkedModulator:
    """chunked-modulator.ts:22-88."""

    def __init__(self, modulator):
        self.modulator = modulator
        self.pendingSignal = None
        self.samplePosition = 0

    def startModulation(self, data):
        if len(data) == 0:
            self._reset()
            return
        self.pendingSignal = np.asarray(self.modulator.modulateData(bytes(data)), dtype=np.float32)
        self.samplePosition = 0

    def getNextSamples(self, sampleCount):
        if self.pendingSignal is None:
            return None
        remaining = len(self.pendingSignal) - self.samplePosition
        if remaining <= 0:
            return None
        n = min(sampleCount, remaining)
        signal = self.pendingSignal[self.samplePosition:self.samplePosition + n].copy()
        self.samplePosition += n
        total = len(self.pendingSignal)
        if self.samplePosition >= total:
            self._reset()
            return {"signal": signal, "isComplete": True, "samplesConsumed": total, "totalSamples": total}
        return {"signal": signal, "isComplete": False, "samplesConsumed": self.samplePosition, "totalSamples": total}

    def isModulating(self):
        return self.pendingSignal is not None

    def getProgress(self):
        return self.samplePosition / len(self.pendingSignal) if self.pendingSignal is not None else 0

    def cancel(self):
        self._reset()

    def _reset(self):
        self.pendingSignal = None
        self.samplePosition = 0


# What FSKProcessorBatch.snapshot() returns: the engine's stream snapshot and the processor's own image, taken at one moment.
ProcessorBatchSnapshot = collections.namedtuple("ProcessorBatchSnapshot", ["engine", "processor"])


def processor_snapshot_concat(blobs):
    """fskhip_processor_snapshot_concat: one processor snapshot holding the records of `blobs` in order, in canonical form -- byte
    for byte the image one processor holding the same streams writes (host only, no device needed).  `bytes`."""
    bs = [_blob(b) for b in blobs]
    L = _lib.lib()
    ptrs = (C.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    sizes = (C.c_size_t * len(bs))(*[b.nbytes for b in bs])
    need = C.c_size_t(0)
    rc = L.fskhip_processor_snapshot_concat(ptrs, sizes, len(bs), None, 0, C.byref(need))
    if rc != _lib.E_OVERFLOW:
        _lib.check(rc)
    out = np.zeros(need.value, np.uint8)
    _lib.check(L.fskhip_processor_snapshot_concat(ptrs, sizes, len(bs), out.ctypes.data, out.nbytes, C.byref(need)))
    return out.tobytes()


def processor_snapshot_info(blob):
    """fskhip_processor_snapshot_info_get: what a processor snapshot holds (validated on the host, no device needed)"""
    b = _blob(blob)
    info = _lib.ProcessorSnapshotInfo()
    _lib.check(_lib.lib().fskhip_processor_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


def rate_handle_check(handle, kind, what, n_streams, device):
    """a side's resampler (filters.Upsampler / Downsampler; `kind`) or the converter of its direction, as a batch of n_streams
    streams on `device` (None: not known) takes it: ValueError otherwise.  FSKProcessorBatch's check, and each shard's of
    FSKProcessorBatchSharded."""
    from . import filters
    converter = {filters.Upsampler: filters.CaptureConverter, filters.Downsampler: filters.PlaybackConverter}[kind]
    if not isinstance(handle, (kind, converter)):     # (a converter of the side's direction stands in its resampler's place)
        raise ValueError("%s must be a filters.%s, got %s" % (what, kind.__name__, type(handle).__name__))
    if handle.n_streams != n_streams:
        raise ValueError("%s has %d streams, the batch %d" % (what, handle.n_streams, n_streams))
    if device is not None and handle.device != device:
        raise ValueError("%s is on device %r, the batch on %r" % (what, handle.device, device))


def rate_call_kind(upsampler, n_in, downsampler, n_out, any_length=False):
    """which library call a rate quantum with these handles is (None: the side has no samples): "rate" for resamplers, "ratecvt"
    for converters, whose counts are whole periods, "ratecvt_any" for converters and counts of any length (any_length; a resampler
    in a slot is a TypeError).  One call takes one kind."""
    from . import filters
    if any_length:
        for what, h in (("upsampler", upsampler), ("downsampler", downsampler)):
            if h is not None and not isinstance(h, filters._RateConverter):
                raise TypeError("%s is a %s: quanta of any length go through rate converters (filters.CaptureConverter / PlaybackConverter)"
                                % (what, type(h).__name__))
        return "ratecvt_any"
    kinds = [isinstance(h, filters._RateConverter) for h in (upsampler, downsampler) if h is not None]
    if len(set(kinds)) > 1:
        raise ValueError("upsampler is a %s and downsampler a %s: one call takes resamplers or rate converters, not one of each"
                         % (type(upsampler).__name__, type(downsampler).__name__))
    if not any(kinds):
        return "rate"
    if upsampler is not None and n_in % upsampler.down:
        raise ValueError("%d samples per stream are not a multiple of the converter's down factor %d" % (n_in, upsampler.down))
    if downsampler is not None and n_out % downsampler.up:
        raise ValueError("n_out %d is not a multiple of the converter's up factor %d" % (n_out, downsampler.up))
    return "ratecvt"


class FSKProcessorBatch:
    """S FSKProcessors over one FSKEngine.  rx_capacity 1024 is the reference's demodulatedBuffer size
    (fsk-processor.ts:84); clear_rx_on_tx_complete mirrors its 'modulate' handler (228-235)."""

    def __init__(self, engine, rx_capacity=1024, clear_rx_on_tx_complete=True, use_graph=False):
        self.engine = engine
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.fskhip_processor_create(engine._h, rx_capacity, C.byref(h)))
        self._h = h
        self.n_streams = engine.n_streams
        self.rx_capacity = rx_capacity
        self.flags = (PROC_CLEAR_RX_ON_TX_COMPLETE if clear_rx_on_tx_complete else 0) | (PROC_GRAPH if use_graph else 0)
        self.processDemodulationCallCount = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_processor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- lifecycle: the processors follow their FSKCores through a remap / a snapshot (include/fskhip_next.h) -------
    def _like(self, engine):
        return FSKProcessorBatch(engine, rx_capacity=self.rx_capacity, clear_rx_on_tx_complete=bool(self.flags & PROC_CLEAR_RX_ON_TX_COMPLETE),
                                 use_graph=bool(self.flags & PROC_GRAPH))

    def remapped(self, stream_map, configs=None, options=None):
        """A new batch of len(stream_map) streams whose stream i continues stream stream_map[i] of this one -- FSKCore
        (engine.remapped) and FSKProcessor (fskhip_processor_remap: ring, pending modulation, completed count) -- or starts
        as a new FSKProcessor where stream_map[i] is -1.  The new batch owns its engine (close both); this batch stays
        usable.  processDemodulationCallCount is carried."""
        m = np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        eng = self.engine.remapped(m, configs=configs, options=options)
        try:
            nxt = self._like(eng)
        except Exception:
            eng.close()
            raise
        try:
            _lib.check(self._L.fskhip_processor_remap(nxt._h, self._h, m.ctypes.data, len(m)))
        except Exception:
            nxt.close()
            eng.close()
            raise
        nxt.processDemodulationCallCount = self.processDemodulationCallCount
        return nxt

    def snapshot(self, streams=None):
        """The pair of images of streams `streams` (None: all, in order): .engine (FSKEngine.snapshot) and .processor
        (fskhip_processor_snapshot), both `bytes`.  The batch is read only and stays usable."""
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int64).reshape(-1)
        n = self.n_streams if sel is None else len(sel)
        sel_p = None if sel is None else sel.ctypes.data
        need = int(self._L.fskhip_processor_snapshot_bytes(self._h, sel_p, n))
        buf = np.zeros(max(need, 1), np.uint8)
        w = C.c_size_t(0)
        _lib.check(self._L.fskhip_processor_snapshot(self._h, sel_p, n, buf.ctypes.data, need, C.byref(w)))
        return ProcessorBatchSnapshot(engine=self.engine.snapshot(streams).tobytes(), processor=buf[:w.value].tobytes())

    @classmethod
    def from_snapshot(cls, snap, stream_map=None, configs=None, device=0, options=None, clear_rx_on_tx_complete=True, use_graph=False):
        """A new batch on `device` that continues the records of a snapshot() pair: stream i continues record stream_map[i]
        of both images (-1: a new FSKCore and FSKProcessor; None: every record, in order).  The engine is made by
        FSKEngine.from_snapshot, which checks the configs; rx_capacity is the image's.  The host counter
        processDemodulationCallCount is not part of an image and starts at 0."""
        info = processor_snapshot_info(snap.processor)
        m = np.arange(info["n_streams"], dtype=np.int64) if stream_map is None else np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        eng = FSKEngine.from_snapshot(snap.engine, stream_map=m, configs=configs, device=device, options=options)
        try:
            nxt = cls(eng, rx_capacity=info["rx_capacity"], clear_rx_on_tx_complete=clear_rx_on_tx_complete, use_graph=use_graph)
        except Exception:
            eng.close()
            raise
        try:
            b = _blob(snap.processor)
            _lib.check(nxt._L.fskhip_processor_restore(nxt._h, b.ctypes.data, b.nbytes, m.ctypes.data, len(m)))
        except Exception:
            nxt.close()
            eng.close()
            raise
        return nxt

    # ---- process(inputs, outputs) fsk-processor.ts:152-167 -----------------------------------------
    def process(self, inputs=None, n_out=0, out=None):
        """inputs: float32 [S, n_in] or None; returns float32 [S, n_out] (or None when n_out == 0).  out: the float32 [S, n_out]
        array to write and return instead of a new one -- its rows may be a block of a wider array (engine.samples_out: anything
        whose dtype, shape or pitch the call cannot express is a ValueError, raised before the call is counted)."""
        out_pitch = n_out
        if out is not None or n_out:
            out, _code, _lay, out_pitch = self._out_array(out, "f32", "stream", n_out)
        x = None
        n_in = 0
        if inputs is not None:
            x = np.ascontiguousarray(inputs, dtype=np.float32)
            if x.ndim != 2 or x.shape[0] != self.n_streams:
                raise ValueError("inputs must be [n_streams, n]")
            n_in = x.shape[1]
            self.processDemodulationCallCount += 1
        # the host form stages through the processor's own stream, which a graph capture needs anyway
        _lib.check(self._L.fskhip_processor_process_host(
            self._h, x.ctypes.data if x is not None else None, n_in, n_in,
            out.ctypes.data if out is not None else None, n_out, out_pitch, self.flags))
        return out

    def _out_array(self, out, out_fmt, out_layout, n_out):
        """engine.samples_out for a quantum's output: a new array, or the caller's `out` checked -- which has to go with an n_out"""
        if out is not None and not n_out:
            raise ValueError("out was given, but n_out is 0: the call writes nothing")
        return samples_out(out_fmt, out_layout, self.n_streams, int(n_out), out)

    def graph_stats(self):
        """fskhip_processor_graph_stats: (captures, replays) -- the quanta use_graph captured afresh and the quanta that replayed
        the capture before them, since the batch was made.  A quantum that ran plainly is in neither."""
        cap, rep = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._L.fskhip_processor_graph_stats(self._h, C.byref(cap), C.byref(rep)))
        return int(cap.value), int(rep.value)

    @property
    def last_tx_kernel(self):
        """fskhip_processor_last_tx_kernel: the kernel that wrote the last quantum's output, or the two launches that stand for one
        joined by '+' ("processor_io_ratecvt_kernel<any>", "processor_io_kernel+ratecvt_playback_any_kernel", ...); "" where the
        quantum had no TX side.  Every process form sets it."""
        return (self._L.fskhip_processor_last_tx_kernel(self._h) or b"").decode()

    def process_device(self, d_in, n_in, in_pitch, d_out, n_out, out_pitch, stream=None, flags=None):
        _lib.check(self._L.fskhip_processor_process_device(self._h, d_in, n_in, in_pitch, d_out, n_out, out_pitch,
                                                           self.flags if flags is None else flags, stream))

    def process_samples(self, inputs=None, in_fmt="f32", in_layout="stream", n_out=0, out_fmt="f32", out_layout="stream", out=None):
        """process() with either side in a capture format (SAMPLE_FORMATS: "f32", "s16", "mulaw", "alaw") and layout
        (SAMPLE_LAYOUTS: "stream" = [S, n], "sample" = [n, S], interleaved frames): fskhip_processor_process_fmt_host.  inputs: an
        array of in_fmt's dtype in in_layout's shape (rows may be a block of a wider array, whose other columns are ignored), or
        None; returns an array of out_fmt's dtype, [S, n_out] or [n_out, S] (None when n_out == 0).  The samples cross PCIe as
        they are; the state ends as process() leaves it on the decoded floats, the output is process()'s, encoded.  out: the
        array of out_fmt's dtype and out_layout's shape to write and return instead of a new one; its rows may be a block of a
        wider array -- a shard's column block of interleaved frames, at the full frame pitch (process(): a ValueError otherwise)."""
        in_code, in_lay = _sample_codes(in_fmt, in_layout)
        out_code, out_lay = _sample_codes(out_fmt, out_layout)      # (every argument check comes before the call is counted)
        x, n_in, in_pitch = None, 0, 0
        if inputs is not None:
            x, in_code, in_lay, S, n_in, in_pitch = sample_args(inputs, in_fmt, in_layout)
            if in_pitch is None:      # (an array without elements has no strides to speak of: its rows are packed)
                in_pitch = max(x.shape[1], 1)
            if S != self.n_streams:
                raise ValueError("inputs must be [n_streams, n] (layout 'stream') or [n, n_streams] (layout 'sample')")
        out_pitch = 0
        if out is not None or n_out:
            out, out_code, out_lay, out_pitch = self._out_array(out, out_fmt, out_layout, n_out)
        if inputs is not None:
            self.processDemodulationCallCount += 1
        _lib.check(self._L.fskhip_processor_process_fmt_host(
            self._h, x.ctypes.data if x is not None else None, in_code, in_lay, n_in, in_pitch,
            out.ctypes.data if out is not None else None, out_code, out_lay, int(n_out), out_pitch, self.flags))
        return out

    def process_samples_device(self, d_in, in_fmt, in_layout, n_in, in_pitch, d_out, out_fmt, out_layout, n_out, out_pitch, stream=None, flags=None):
        """fskhip_processor_process_fmt_device: device pointers (ints or None), pitches in elements, asynchronous on `stream`"""
        _lib.check(self._L.fskhip_processor_process_fmt_device(self._h, d_in, *_sample_codes(in_fmt, in_layout, True), n_in, in_pitch,
                                                               d_out, *_sample_codes(out_fmt, out_layout, True), n_out, out_pitch,
                                                               self.flags if flags is None else flags, stream))

    def _rate_handle(self, handle, kind, what):
        """a side's resampler (filters.Upsampler / Downsampler) as fskhip_processor_process_rate_* wants it: of this batch's
        stream count and on its engine's device"""
        rate_handle_check(handle, kind, what, self.n_streams, getattr(self.engine, "device", None))
        return handle._h

    def _rate_entry(self, form, upsampler, n_in, downsampler, n_out, any_length=False):
        """the library call of form "host" / "device" for the handles of the sides that have samples (None: the side has none):
        fskhip_processor_process_rate_* for resamplers, fskhip_processor_process_ratecvt_* for converters (filters.CaptureConverter /
        PlaybackConverter), whose counts are whole periods.  One call takes one kind.  any_length: the converters' call for
        counts of any length, fskhip_processor_process_ratecvt_any_*; a resampler in a slot is a TypeError."""
        return getattr(self._L, "fskhip_processor_process_%s_%s" % (rate_call_kind(upsampler, n_in, downsampler, n_out, any_length), form))

    def process_samples_at(self, inputs=None, in_fmt="mulaw", in_layout="sample", upsampler=None, n_out=0, out_fmt="mulaw", out_layout="sample",
                           downsampler=None, out=None):
        """process_samples() with both sides at the trunk's own rate: fskhip_processor_process_rate_host.  inputs (or None) are
        low rate samples, interpolated on the device by `upsampler` (filters.Upsampler) in front of the demodulator; the n_out
        returned samples are the pending modulation decimated by `downsampler` (filters.Downsampler), which one kernel generates,
        filters and encodes.  Both handles carry their histories from call to call, so any cut of a stream into quanta gives the
        same bytes and samples; the state ends as Upsampler.process -> process() -> Downsampler.process leaves it, bit for bit.
        A side without samples needs no handle.

        With a filters.CaptureConverter as `upsampler` and a filters.PlaybackConverter as `downsampler` both sides are at the
        converters' outer rate -- 44.1 kHz either side of a 48 kHz engine -- through fskhip_processor_process_ratecvt_host: the
        inputs are a multiple of the capture converter's `down` samples per stream, n_out a multiple of the playback
        converter's `up`, and the state ends as CaptureConverter.process -> process() -> PlaybackConverter.process leaves it,
        bit for bit.  One call takes resamplers or converters, not one of each.  out: as in process_samples()."""
        return self._samples_at(False, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out)

    def _samples_at(self, any_length, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out=None):
        """process_samples_at (any_length False) and process_samples_at_any: the host form behind their argument checks"""
        from . import filters
        in_code, in_lay = _sample_codes(in_fmt, in_layout)
        out_code, out_lay = _sample_codes(out_fmt, out_layout)      # (every argument check comes before the call is counted)
        x, n_in, in_pitch, up_h, down_h = None, 0, 0, None, None
        if inputs is not None:
            x, in_code, in_lay, S, n_in, in_pitch = sample_args(inputs, in_fmt, in_layout)
            if in_pitch is None:      # (an array without elements has no strides to speak of: its rows are packed)
                in_pitch = max(x.shape[1], 1)
            if S != self.n_streams:
                raise ValueError("inputs must be [n_streams, n] (layout 'stream') or [n, n_streams] (layout 'sample')")
            up_h = self._rate_handle(upsampler, filters.Upsampler, "upsampler")
        if n_out:
            down_h = self._rate_handle(downsampler, filters.Downsampler, "downsampler")
        entry = self._rate_entry("host", upsampler if inputs is not None else None, n_in, downsampler if n_out else None, int(n_out), any_length)
        out_pitch = 0
        if out is not None or n_out:
            out, out_code, out_lay, out_pitch = self._out_array(out, out_fmt, out_layout, n_out)
        if inputs is not None:
            self.processDemodulationCallCount += 1
        _lib.check(entry(
            self._h, up_h, down_h, x.ctypes.data if x is not None else None, in_code, in_lay, n_in, in_pitch,
            out.ctypes.data if out is not None else None, out_code, out_lay, int(n_out), out_pitch, self.flags))
        return out

    def process_samples_at_any(self, inputs=None, in_fmt="mulaw", in_layout="sample", upsampler=None, n_out=0, out_fmt="mulaw", out_layout="sample",
                               downsampler=None, out=None):
        """process_samples_at() through a filters.CaptureConverter and a filters.PlaybackConverter for quanta of any length -- a
        WebAudio render quantum of 128 frames at 44.1 kHz as it arrives: fskhip_processor_process_ratecvt_any_host.  The handles
        carry their positions (filters: `position`) from call to call beside their histories; the state ends as
        CaptureConverter.process_any -> process() with the engine counts the handles give (upsampler.out_count_any(n),
        downsampler.in_count_any(n_out); a side with none is left out) -> PlaybackConverter.process_any leaves it, bit for bit.
        An n_out that the playback converter cannot write from its position (only where its up > down) is the library's refusal.
        A resampler in a slot is a TypeError.  out: as in process_samples()."""
        return self._samples_at(True, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out)

    def process_samples_at_any_device(self, d_in, in_fmt, in_layout, n_in, in_pitch, upsampler, d_out, out_fmt, out_layout, n_out, out_pitch, downsampler,
                                      stream=None, flags=None):
        """fskhip_processor_process_ratecvt_any_device: process_samples_at_device for converters and counts of any length"""
        self._samples_at_device(True, d_in, in_fmt, in_layout, n_in, in_pitch, upsampler, d_out, out_fmt, out_layout, n_out, out_pitch, downsampler, stream, flags)

    def process_samples_at_device(self, d_in, in_fmt, in_layout, n_in, in_pitch, upsampler, d_out, out_fmt, out_layout, n_out, out_pitch, downsampler,
                                  stream=None, flags=None):
        """fskhip_processor_process_rate_device: device pointers (ints or None), lengths and pitches in low rate elements,
        asynchronous on `stream`.  The handle of a side whose pointer is None may be None.  With converters
        (filters.CaptureConverter / PlaybackConverter) it is fskhip_processor_process_ratecvt_device, as in process_samples_at."""
        self._samples_at_device(False, d_in, in_fmt, in_layout, n_in, in_pitch, upsampler, d_out, out_fmt, out_layout, n_out, out_pitch, downsampler, stream, flags)

    def _samples_at_device(self, any_length, d_in, in_fmt, in_layout, n_in, in_pitch, upsampler, d_out, out_fmt, out_layout, n_out, out_pitch, downsampler, stream, flags):
        """process_samples_at_device (any_length False) and process_samples_at_any_device"""
        from . import filters
        up_h = None if d_in is None and upsampler is None else self._rate_handle(upsampler, filters.Upsampler, "upsampler")
        down_h = None if d_out is None and downsampler is None else self._rate_handle(downsampler, filters.Downsampler, "downsampler")
        entry = self._rate_entry("device", None if d_in is None else upsampler, n_in, None if d_out is None else downsampler, n_out, any_length)
        _lib.check(entry(self._h, up_h, down_h, d_in, *_sample_codes(in_fmt, in_layout, True), n_in, in_pitch,
                         d_out, *_sample_codes(out_fmt, out_layout, True), n_out, out_pitch, self.flags if flags is None else flags, stream))

    # ---- 'modulate' fsk-processor.ts:87-113 ------------------------------------------------------------
    def modulate(self, payloads, mask=None):
        """payloads: list of S bytes-like; mask: optional list of S bools (streams to start)."""
        rows = [bytes(p) for p in payloads]
        if len(rows) != self.n_streams:
            raise ValueError("need one payload per stream")
        lens = np.array([len(r) for r in rows], dtype=np.uint32)
        pitch = max(1, int(lens.max()))
        slab = np.zeros((self.n_streams, pitch), dtype=np.uint8)
        for i, r in enumerate(rows):
            slab[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
        rc = self._L.fskhip_processor_modulate_host(self._h, slab.ctypes.data, lens.ctypes.data, pitch,
                                                    m.ctypes.data if m is not None else None)
        _lib.check_busy(rc, "Modulation already in progress")  # fsk-processor.ts:91

    def tx_state(self):
        S = self.n_streams
        pos, total, done = (np.zeros(S, np.uint32) for _ in range(3))
        pend = np.zeros(S, np.uint8)
        _lib.check(self._L.fskhip_processor_tx_state_host(self._h, pos.ctypes.data, total.ctypes.data, pend.ctypes.data,
                                                          done.ctypes.data))
        return {"samplePosition": pos, "totalSamples": total, "pendingModulation": pend.astype(bool), "completed": done,
                "isModulating": total > 0,
                "progress": np.where(total > 0, pos / np.maximum(total, 1), 0.0)}

    # ---- 'demodulate' fsk-processor.ts:117-138 (without the wait) -----------------------------------------
    def demodulate(self):
        out = np.zeros((self.n_streams, self.rx_capacity), dtype=np.uint8)
        counts = np.zeros(self.n_streams, dtype=np.uint32)
        _lib.check(self._L.fskhip_processor_rx_drain_host(self._h, out.ctypes.data, self.rx_capacity, counts.ctypes.data))
        return [out[s, :counts[s]].tobytes() for s in range(self.n_streams)]

    def demodulate_sparse(self, mask=None, min_len=1):
        """The same for the streams that hold bytes only (fskhip_processor_rx_drain_sparse_host): (streams, offsets, data) --
        the streams with at least max(min_len, 1) buffered bytes (and mask[s], where a mask is given) in ascending order, and
        their bytes in CSR form: those of streams[i] are data[offsets[i]:offsets[i + 1]], oldest first.  uint32, uint32
        (one entry more than streams) and uint8 arrays of exactly the returned sizes.  Streams not listed keep their rings."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(-1).astype(np.uint8))
            if len(m) != self.n_streams:
                raise ValueError("mask must have one entry per stream")
        m_p = None if m is None else m.ctypes.data
        na, nb = C.c_uint32(0), C.c_uint32(0)
        # a size query first: an overflowing call drains nothing, so the second call finds what the first one counted
        rc = self._L.fskhip_processor_rx_drain_sparse_host(self._h, m_p, min_len, None, None, 0, None, 0, C.byref(na), C.byref(nb))
        if rc != _lib.E_OVERFLOW:
            _lib.check(rc)
        streams = np.zeros(na.value, np.uint32)
        offsets = np.zeros(na.value + 1, np.uint32)
        data = np.zeros(nb.value, np.uint8)
        if rc == _lib.E_OVERFLOW:
            _lib.check(self._L.fskhip_processor_rx_drain_sparse_host(self._h, m_p, min_len, streams.ctypes.data, offsets.ctypes.data, na.value,
                                                                     data.ctypes.data, nb.value, C.byref(na), C.byref(nb)))
        return streams, offsets, data

    def demodulate_active(self, mask=None, min_len=1):
        """demodulate_sparse as {stream: bytes} of the streams that held any."""
        streams, offsets, data = self.demodulate_sparse(mask=mask, min_len=min_len)
        return {int(s): data[offsets[i]:offsets[i + 1]].tobytes() for i, s in enumerate(streams)}

    def rx_lengths(self):
        lens = np.zeros(self.n_streams, dtype=np.uint32)
        _lib.check(self._L.fskhip_processor_rx_length_host(self._h, lens.ctypes.data))
        return lens

    def reset(self, stream=-1):
        _lib.check(self._L.fskhip_processor_reset(self._h, stream))

    def status(self, stream=0):
        """The 'status' reply (fsk-processor.ts:240-253) for one stream."""
        st = self.engine.get_status(stream)
        tx = self.tx_state()
        st.update(demodulatedBufferLength=int(self.rx_lengths()[stream]), pendingModulation=bool(tx["pendingModulation"][stream]),
                  fskCoreReady=True, processDemodulationCallCount=self.processDemodulationCallCount)
        return st
