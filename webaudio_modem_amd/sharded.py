"""One host process driving several GPUs: FSKEngineSharded = one FSKEngine per device, each owning a contiguous block
of streams (sharding.stream_shard), calls fanned out on worker threads (libfskhip.so releases nothing Python-side: ctypes
drops the GIL for the duration of a call, every entry point selects its engine's device first, and the library's error
text is thread-local).  The data path still has no collective: streams are independent.

This is the in-process alternative to bench.py's one-process-per-GPU layout, for hosts that own all the node's streams in
one address space (the reference's FSKCore instances live in one JavaScript realm).  napi/fsk-core.js has the same class
(FSKBatchSharded) over the asynchronous N-API calls."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import PRECISION_F32
from .engine import FSKEngine, snapshot_concat, _snapshot_plan, _sample_codes, sample_args, samples_out
from .processor import (FSKProcessorBatch, ProcessorBatchSnapshot, processor_snapshot_concat, processor_snapshot_info, rate_handle_check,
                        rate_call_kind)
from .sharding import all_shards


MAX_WORKERS = 16     # worker threads of one sharded batch: one per shard, and never more than this


class _Sharded:
    """What the sharded classes share: the shard table (`shards`: (first stream, count, device) per shard that has streams), the
    worker pool and the fan-out.  A subclass names its per-shard objects in _units()."""

    def _shard_setup(self, n_streams, devices, first_config):
        """`devices` as a list (None: every HIP device of the node; first_config: what the loud failure on a box without one is
        made with) and the shard table over it: sharding.all_shards' contiguous blocks, devices with nothing to do left out"""
        if devices is None:
            n_dev = int(_lib.lib().fskhip_device_count())
            if n_dev <= 0:
                # same loud failure as FSKEngine on a box without a GPU: there is no CPU path
                FSKEngine(1, first_config)
            devices = list(range(max(n_dev, 1)))
        devices = list(devices)
        if not devices:
            raise ValueError("no devices")
        self.n_streams = n_streams
        self.devices = devices
        self.shards = [(first, count, dev) for (first, count), dev in zip(all_shards(n_streams, len(devices)), devices) if count]
        self._pool = None

    def _start_pool(self):
        self._pool = ThreadPoolExecutor(max_workers=min(MAX_WORKERS, max(1, len(self.shards))), thread_name_prefix="fskhip-dev")

    def _stop_pool(self):
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=True)
            self._pool = None

    def locate(self, stream):
        """(shard index, local stream index) of a global stream index."""
        if not (0 <= stream < self.n_streams):
            raise ValueError("stream out of range")
        for i, (first, count, _dev) in enumerate(self.shards):
            if first <= stream < first + count:
                return i, stream - first
        raise AssertionError("unreachable")

    def _fan_out(self, fn):
        """fn(shard index, the shard's object, first, count) on every shard concurrently; results in shard order.  The first
        exception is re-raised after every worker has finished (no call is left running on a device)."""
        futs = [self._pool.submit(fn, i, u, self.shards[i][0], self.shards[i][1]) for i, u in enumerate(self._units())]
        results, err = [], None
        for f in futs:
            try:
                results.append(f.result())
            except Exception as ex:  # noqa: BLE001 -- collected, re-raised below
                err = err or ex
                results.append(None)
        if err is not None:
            raise err
        return results


class FSKEngineSharded(_Sharded):
    """S independent FSKCore instances spread over `devices` (default: every HIP device of the node).

    Same methods as FSKEngine where a host-side call makes sense for a sharded batch; stream indices are global.
    engine_factory(count, configs, device, precision) -> engine is there for tests (no GPU needed to check the
    shard / gather logic)."""

    def __init__(self, n_streams, configs=None, devices=None, precision=PRECISION_F32, engine_factory=None):
        if devices is None and engine_factory is not None:
            # a stand-in engine (CPU tests of the sharding / gather logic): the HIP library is not touched at all
            raise ValueError("pass `devices` together with an engine_factory")
        if isinstance(configs, (list, tuple)) and len(configs) != n_streams:
            raise ValueError("need one config per stream")
        make = engine_factory or (lambda count, cfg, dev, prec: FSKEngine(count, cfg, device=dev, precision=prec))
        self._factory = engine_factory
        self.precision = precision
        # devices with nothing to do (more devices than streams) get no engine
        self._shard_setup(n_streams, devices, configs if not isinstance(configs, (list, tuple)) else configs[0])
        self.engines = []
        try:
            for first, count, dev in self.shards:
                cfg = list(configs[first:first + count]) if isinstance(configs, (list, tuple)) else configs
                self.engines.append(make(count, cfg, dev, precision))
        except Exception:
            self.close()
            raise
        self._start_pool()

    def _units(self):
        return self.engines

    # ---- plumbing --------------------------------------------------------------------------------
    def close(self):
        for e in getattr(self, "engines", []):
            e.close()
        self.engines = []
        self._stop_pool()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stream snapshots: checkpoint, grow, shrink and rebalance a sharded batch (include/fskhip.h) -------------------
    # These need engines that implement snapshot() / restore_from(): real FSKEngines, or an engine_factory stand-in that has
    # the two methods (stand-ins without them keep serving every other method).
    def snapshot(self):
        """One snapshot of the whole batch, records in global stream order: every shard's snapshot, concatenated
        (fskhip_snapshot_concat: the shards were created together and fed the same calls, so they are images of what could
        have been one engine)."""
        parts = self._fan_out(lambda i, e, first, count: e.snapshot())
        return parts[0] if len(parts) == 1 else snapshot_concat(parts)

    @classmethod
    def from_snapshot(cls, blob, stream_map=None, configs=None, devices=None, engine_factory=None):
        """A new sharded batch whose stream i continues record stream_map[i] of the snapshot (-1: a new FSKCore; None: every
        record in order), spread over `devices`: every shard restores its slice of the map from the one blob.  Precision and
        configs come from the snapshot unless `configs` is given (a -1 slot needs one when the snapshot's are per stream)."""
        info, m, configs = _snapshot_plan(blob, stream_map, configs, range_error=False)   # (an entry past the records: the library refuses it)
        new = cls(len(m), configs, devices=devices, precision=info["precision"], engine_factory=engine_factory)
        try:
            new._fan_out(lambda i, e, first, count: e.restore_from(blob, m[first:first + count]))
        except Exception:
            new.close()
            raise
        return new

    def remapped(self, stream_map, configs=None, devices=None):
        """A new sharded batch of len(stream_map) streams on `devices` (default: this batch's) whose stream i continues
        GLOBAL stream stream_map[i] of this one, or starts as a new FSKCore where it is -1 -- across shards and devices: the
        state goes through one host-side snapshot.  This batch is left as it is (close it when the new one has taken over)."""
        return type(self).from_snapshot(self.snapshot(), stream_map, configs=configs, devices=self.devices if devices is None else devices,
                                        engine_factory=self._factory)

    # ---- demodulateData / modulateData (fsk.ts:190-222, 377-424) ---------------------------------
    def demodulate_data(self, samples, writeback_agc=False):
        """samples: float32 [S, N] (host).  Returns (list of bytes per stream, eod counts ndarray), stream order."""
        x = samples if (isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous) \
            else np.ascontiguousarray(samples, dtype=np.float32)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.shape[0] != self.n_streams:
            raise ValueError("expected %d streams, got %d" % (self.n_streams, x.shape[0]))
        parts = self._fan_out(lambda i, e, first, count: e.demodulate_data(x[first:first + count], writeback_agc=writeback_agc))
        out, eod = [], []
        for o, c in parts:
            out.extend(o)
            eod.append(np.asarray(c, dtype=np.uint32))
        if writeback_agc and x is not samples:
            np.copyto(samples, x.reshape(np.shape(samples)))
        return out, (np.concatenate(eod) if eod else np.zeros(0, np.uint32))

    def demodulate_samples(self, samples, fmt=None, layout="stream", out_pitch=None):
        """FSKEngine.demodulate_samples over the shards.  No host copy: a shard's streams are a row block of a stream-major
        array, and a COLUMN block of interleaved frames -- its first column's address and the full frame pitch."""
        x, code, lay, S, _N, _pitch = sample_args(samples, fmt, layout)
        if S != self.n_streams:
            raise ValueError("expected %d streams, got %d" % (self.n_streams, S))
        sample_major = lay == _lib.LAYOUT_SAMPLE_MAJOR
        parts = self._fan_out(lambda i, e, first, count: e.demodulate_samples(
            x[:, first:first + count] if sample_major else x[first:first + count], fmt=code, layout=lay, out_pitch=out_pitch))
        out, eod = [], []
        for o, c in parts:
            out.extend(o)
            eod.append(np.asarray(c, dtype=np.uint32))
        return out, (np.concatenate(eod) if eod else np.zeros(0, np.uint32))

    def modulate_data(self, payloads):
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        parts = self._fan_out(lambda i, e, first, count: e.modulate_data(payloads[first:first + count]))
        return [sig for p in parts for sig in p]

    def modulate_samples(self, payloads, fmt, layout="stream", n_per_stream=None, out=None):
        """FSKEngine.modulate_samples over the shards: ONE array for the whole batch and no host copy -- every shard writes its row
        block of a stream-major array, or its COLUMN block of the interleaved frames at the full frame pitch."""
        if len(payloads) != self.n_streams:
            raise ValueError("need one payload per stream")
        if n_per_stream is None:   # (one signal length per payload size: the fields it depends on are shared by every stream)
            n_per_stream = self.engines[0].modulated_length(max((len(p) for p in payloads), default=0))
        n = int(n_per_stream)
        out, code, lay, _pitch = samples_out(fmt, layout, self.n_streams, n, out)
        sample_major = lay == _lib.LAYOUT_SAMPLE_MAJOR
        parts = self._fan_out(lambda i, e, first, count: e.modulate_samples(
            payloads[first:first + count], code, lay, n_per_stream=n, out=out[:, first:first + count] if sample_major else out[first:first + count])[1])
        return out, (np.concatenate([np.asarray(p, dtype=np.uint32) for p in parts]) if parts else np.zeros(0, np.uint32))

    # ---- reset / getStatus -----------------------------------------------------------------------
    def reset(self, stream=-1):
        if stream < 0:
            self._fan_out(lambda i, e, first, count: e.reset(-1))
        else:
            i, local = self.locate(stream)
            self.engines[i].reset(local)

    def get_status(self, stream=0):
        i, local = self.locate(stream)
        return self.engines[i].get_status(local)

    def demod_supported(self):
        return all(e.demod_supported() for e in self.engines)


class FSKProcessorBatchSharded(_Sharded):
    """S FSKProcessors spread over `devices` (default: every HIP device of the node): one FSKEngine and one FSKProcessorBatch per
    device over sharding.all_shards' contiguous blocks, a streaming quantum fanned out on worker threads as FSKEngineSharded fans
    out its calls.  The methods are FSKProcessorBatch's, stream indices are global, and a quantum costs no host copy: a shard
    reads its row block of a stream-major input, or its column block of interleaved frames at the full frame pitch, and writes its
    block of ONE output array for the whole batch.  The hot path is the per-shard launches, unchanged.

    `engines` and `processors` are the per-shard objects (XModem handles are built on `processors`, shard by shard).  The rate
    forms take one handle per shard (make_rate_handles).  snapshot / from_snapshot / remapped move live processors between
    devices: the shards' images go under one header (snapshot_concat, processor_snapshot_concat) and every shard of the new batch
    restores its slice of the map from that one pair.

    processor_factory(count, configs, device, precision) -> processor is there for tests (no GPU needed to check the shard /
    gather logic): a stand-in with the methods of FSKProcessorBatch that the test calls, and `engine` if it has one."""

    def __init__(self, n_streams, configs=None, devices=None, precision=PRECISION_F32, rx_capacity=1024, clear_rx_on_tx_complete=True, use_graph=False,
                 options=None, processor_factory=None):
        def make(i, first, count, dev):
            cfg = list(configs[first:first + count]) if isinstance(configs, (list, tuple)) else configs
            if processor_factory is not None:
                return processor_factory(count, cfg, dev, precision)
            eng = FSKEngine(count, cfg, device=dev, precision=precision, options=options)
            try:
                return FSKProcessorBatch(eng, rx_capacity=rx_capacity, clear_rx_on_tx_complete=clear_rx_on_tx_complete, use_graph=use_graph)
            except Exception:
                eng.close()
                raise
        if isinstance(configs, (list, tuple)) and len(configs) != n_streams:
            raise ValueError("need one config per stream")
        self._build(n_streams, configs, devices, precision, rx_capacity, clear_rx_on_tx_complete, use_graph, options, processor_factory, make)

    def _build(self, n_streams, configs, devices, precision, rx_capacity, clear_rx_on_tx_complete, use_graph, options, processor_factory, make):
        """the shard table, then make(shard index, first, count, device) -> processor for every shard, one after the other"""
        if devices is None and processor_factory is not None:
            # stand-in processors (CPU tests of the sharding / gather logic): the HIP library is not touched at all
            raise ValueError("pass `devices` together with a processor_factory")
        self._factory = processor_factory
        self.precision, self.rx_capacity, self.options = precision, rx_capacity, options
        self.clear_rx_on_tx_complete, self.use_graph = bool(clear_rx_on_tx_complete), bool(use_graph)
        self.processDemodulationCallCount = 0
        self.processors = []
        self._shard_setup(n_streams, devices, configs[0] if isinstance(configs, (list, tuple)) and configs else configs)
        try:
            for i, (first, count, dev) in enumerate(self.shards):
                self.processors.append(make(i, first, count, dev))
        except Exception:
            self.close()
            raise
        self._start_pool()

    def _units(self):
        return self.processors

    @property
    def engines(self):
        """the shards' FSKEngines (None for a stand-in processor without one)"""
        return [getattr(p, "engine", None) for p in self.processors]

    def close(self):
        for p in getattr(self, "processors", []):
            eng = getattr(p, "engine", None)
            p.close()
            if eng is not None:
                eng.close()
        self.processors = []
        self._stop_pool()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- lifecycle: one pair of images for the whole batch ---------------------------------------------------------------
    def snapshot(self):
        """ProcessorBatchSnapshot of the whole batch, records in global stream order: .engine is snapshot_concat of the shards'
        stream snapshots, .processor is processor_snapshot_concat of their processor images -- byte for byte the image one
        FSKProcessorBatch holding the same streams writes.  The batch is read only and stays usable."""
        parts = self._fan_out(lambda i, p, first, count: p.snapshot())
        if len(parts) == 1:
            return ProcessorBatchSnapshot(engine=bytes(parts[0].engine), processor=bytes(parts[0].processor))
        return ProcessorBatchSnapshot(engine=snapshot_concat([s.engine for s in parts]).tobytes(),
                                      processor=processor_snapshot_concat([s.processor for s in parts]))

    @classmethod
    def from_snapshot(cls, snap, stream_map=None, configs=None, devices=None, options=None, clear_rx_on_tx_complete=True, use_graph=False,
                      processor_factory=None):
        """A new sharded batch whose stream i continues record stream_map[i] of a snapshot() pair -- a sharded batch's or a
        single FSKProcessorBatch's -- (-1: a new FSKCore and FSKProcessor; None: every record in order), spread over `devices`:
        every shard restores its slice of the map from the one pair (FSKProcessorBatch.from_snapshot).  Precision, configs and
        rx_capacity are the snapshot's unless `configs` is given.  processDemodulationCallCount starts at 0.  A stand-in made by
        processor_factory takes its slice through restore_from(snap, map)."""
        info, m, configs = _snapshot_plan(snap.engine, stream_map, configs, range_error=False)   # (an entry past the records: the library refuses it)
        pinfo = processor_snapshot_info(snap.processor)
        if pinfo["n_streams"] != info["n_streams"]:
            raise ValueError("the pair's images differ in their record count (engine %d, processor %d): not taken at one moment" % (info["n_streams"], pinfo["n_streams"]))

        def make(i, first, count, dev):
            cfg = list(configs[first:first + count]) if isinstance(configs, (list, tuple)) else configs
            if processor_factory is not None:
                p = processor_factory(count, cfg, dev, info["precision"])
                p.restore_from(snap, m[first:first + count])
                return p
            return FSKProcessorBatch.from_snapshot(snap, stream_map=m[first:first + count], configs=cfg, device=dev, options=options,
                                                   clear_rx_on_tx_complete=clear_rx_on_tx_complete, use_graph=use_graph)
        new = cls.__new__(cls)
        new._build(len(m), configs, devices, info["precision"], pinfo["rx_capacity"], clear_rx_on_tx_complete, use_graph, options, processor_factory, make)
        return new

    def remapped(self, stream_map, configs=None, devices=None):
        """A new sharded batch of len(stream_map) streams on `devices` (default: this batch's) whose stream i continues GLOBAL
        stream stream_map[i] of this one -- FSKCore and FSKProcessor: ring, pending modulation, completed count -- or starts as
        a new one where it is -1, across shards and devices: the state goes through one host-side snapshot() pair.  This batch is
        left as it is (close it when the new one has taken over).  processDemodulationCallCount is carried."""
        new = type(self).from_snapshot(self.snapshot(), stream_map, configs=configs, devices=self.devices if devices is None else devices,
                                       options=self.options, clear_rx_on_tx_complete=self.clear_rx_on_tx_complete, use_graph=self.use_graph,
                                       processor_factory=self._factory)
        new._carry_count(self.processDemodulationCallCount)
        return new

    def _carry_count(self, n):
        self.processDemodulationCallCount = n
        for p in self.processors:
            p.processDemodulationCallCount = n

    # ---- process(inputs, outputs) ---------------------------------------------------------------------------------------
    def _blocks(self, x, sample_major):
        """shard -> its block of a whole-batch array (None: None): rows of a stream-major one, columns of interleaved frames"""
        if x is None:
            return lambda first, count: None
        return (lambda first, count: x[:, first:first + count]) if sample_major else (lambda first, count: x[first:first + count])

    def process(self, inputs=None, n_out=0, out=None):
        """FSKProcessorBatch.process over the shards: inputs float32 [S, n_in] or None; returns float32 [S, n_out] (`out`, where
        given), every shard writing its rows."""
        x = None
        if inputs is not None:
            x = inputs if isinstance(inputs, np.ndarray) and inputs.dtype == np.float32 and inputs.flags.c_contiguous else np.ascontiguousarray(inputs, dtype=np.float32)
            if x.ndim != 2 or x.shape[0] != self.n_streams:
                raise ValueError("inputs must be [n_streams, n]")
        if out is not None and not n_out:
            raise ValueError("out was given, but n_out is 0: the call writes nothing")
        if n_out:
            out = samples_out("f32", "stream", self.n_streams, int(n_out), out)[0]
        xin, xout = self._blocks(x, False), self._blocks(out, False)
        if inputs is not None:       # (counted where every shard counts: behind the argument checks, in front of the call)
            self.processDemodulationCallCount += 1
        self._fan_out(lambda i, p, first, count: p.process(xin(first, count), n_out, out=xout(first, count)))
        return out

    def _samples_args(self, inputs, in_fmt, in_layout, n_out, out_fmt, out_layout, out):
        """the whole-batch arrays of a format quantum, checked: (input or None, its format, layout, samples per stream, output or
        None, its format, layout)"""
        in_code, in_lay = _sample_codes(in_fmt, in_layout)
        out_code, out_lay = _sample_codes(out_fmt, out_layout)
        x, n_in = None, 0
        if inputs is not None:
            x, in_code, in_lay, S, n_in, _pitch = sample_args(inputs, in_fmt, in_layout)
            if S != self.n_streams:
                raise ValueError("inputs must be [n_streams, n] (layout 'stream') or [n, n_streams] (layout 'sample')")
        if out is not None and not n_out:
            raise ValueError("out was given, but n_out is 0: the call writes nothing")
        if n_out:
            out = samples_out(out_code, out_lay, self.n_streams, int(n_out), out)[0]
        return x, in_code, in_lay, n_in, out, out_code, out_lay

    def process_samples(self, inputs=None, in_fmt="f32", in_layout="stream", n_out=0, out_fmt="f32", out_layout="stream", out=None):
        """FSKProcessorBatch.process_samples over the shards, no host copy: a shard's streams are a row block of a stream-major
        array and a COLUMN block of interleaved frames -- its first column's address and the full frame pitch -- on both sides."""
        x, in_code, in_lay, _n_in, out, out_code, out_lay = self._samples_args(inputs, in_fmt, in_layout, n_out, out_fmt, out_layout, out)
        xin, xout = self._blocks(x, in_lay == _lib.LAYOUT_SAMPLE_MAJOR), self._blocks(out, out_lay == _lib.LAYOUT_SAMPLE_MAJOR)
        if inputs is not None:
            self.processDemodulationCallCount += 1
        self._fan_out(lambda i, p, first, count: p.process_samples(xin(first, count), in_code, in_lay, n_out, out_code, out_lay, out=xout(first, count)))
        return out

    def make_rate_handles(self, cls, *args, **kw):
        """One rate handle per shard for the rate forms: cls (filters.Upsampler / Downsampler / CaptureConverter /
        PlaybackConverter) built with *args -- what stands before n_streams: the factor, or the two rates -- and **kw, each with
        its shard's stream count and on its shard's device."""
        made = []
        try:
            for _first, count, dev in self.shards:
                made.append(cls(*args, n_streams=count, device=dev, **kw))
        except Exception:
            for h in made:
                h.close()
            raise
        return made

    def _rate_handles(self, handles, kind, what, n):
        """a side's handles, one per shard, checked as FSKProcessorBatch checks its one -- before any shard is called.  None for a
        side without samples."""
        if not n:
            return [None] * len(self.shards)
        if handles is None or not hasattr(handles, "__len__") or len(handles) != len(self.shards):
            raise ValueError("%s must be a sequence of %d handles, one per shard%s" % (what, len(self.shards), "" if handles is None or not hasattr(handles, "__len__")
                                                                                      else ", got %d" % len(handles)))
        handles = list(handles)
        for h, (_first, count, dev) in zip(handles, self.shards):
            rate_handle_check(h, kind, what, count, dev)
        return handles

    def _samples_at(self, any_length, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out):
        from . import filters
        x, in_code, in_lay, n_in, out, out_code, out_lay = self._samples_args(inputs, in_fmt, in_layout, n_out, out_fmt, out_layout, out)
        ups = self._rate_handles(upsampler, filters.Upsampler, "upsampler", inputs is not None)
        downs = self._rate_handles(downsampler, filters.Downsampler, "downsampler", n_out)
        for u, d in zip(ups, downs):
            rate_call_kind(u, n_in, d, int(n_out), any_length)    # (the single class's refusals, for every shard before any is called)
        if any_length:
            for what, hs in (("upsampler", ups), ("downsampler", downs)):
                pos = [h.position for h in hs if h is not None]
                if len(set(pos)) > 1:
                    raise ValueError("the %s handles stand at different positions %r: the shards of one batch are fed the same calls" % (what, pos))
        xin, xout = self._blocks(x, in_lay == _lib.LAYOUT_SAMPLE_MAJOR), self._blocks(out, out_lay == _lib.LAYOUT_SAMPLE_MAJOR)
        name = "process_samples_at_any" if any_length else "process_samples_at"
        if inputs is not None:
            self.processDemodulationCallCount += 1
        self._fan_out(lambda i, p, first, count: getattr(p, name)(xin(first, count), in_code, in_lay, ups[i], n_out, out_code, out_lay, downs[i],
                                                                   out=xout(first, count)))
        return out

    def process_samples_at(self, inputs=None, in_fmt="mulaw", in_layout="sample", upsampler=None, n_out=0, out_fmt="mulaw", out_layout="sample",
                           downsampler=None, out=None):
        """FSKProcessorBatch.process_samples_at over the shards.  upsampler / downsampler: a sequence of handles, one per shard
        (make_rate_handles), each of its shard's stream count and on its device -- resamplers, or rate converters.  A wrong count
        of handles, stream count or device is a ValueError raised before any shard is called: no state moves."""
        return self._samples_at(False, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out)

    def process_samples_at_any(self, inputs=None, in_fmt="mulaw", in_layout="sample", upsampler=None, n_out=0, out_fmt="mulaw", out_layout="sample",
                               downsampler=None, out=None):
        """FSKProcessorBatch.process_samples_at_any over the shards: sequences of filters.CaptureConverter / PlaybackConverter,
        one per shard, which must all stand at the same `position` (they have been fed the same calls)."""
        return self._samples_at(True, inputs, in_fmt, in_layout, upsampler, n_out, out_fmt, out_layout, downsampler, out)

    @property
    def last_tx_kernel(self):
        """FSKProcessorBatch.last_tx_kernel of every shard, in shard order"""
        return [p.last_tx_kernel for p in self.processors]

    # ---- 'modulate', 'demodulate', reset, 'status' ----------------------------------------------------------------------
    def modulate(self, payloads, mask=None):
        """FSKProcessorBatch.modulate over the shards.  As there, a masked stream with a modulation pending refuses the whole
        call ("Modulation already in progress") and nothing starts -- on any shard: with more than one shard every shard's
        tx_state() is asked first (one more round trip per shard and call), and the RuntimeError's text is this wrapper's, without
        the stream number the library's has; a batch of one shard leaves the refusal to its processor."""
        rows = [bytes(p) for p in payloads]
        if len(rows) != self.n_streams:
            raise ValueError("need one payload per stream")
        m = None
        if mask is not None:
            m = np.asarray(mask, dtype=bool).reshape(-1)
            if len(m) != self.n_streams:
                raise ValueError("mask must have one entry per stream")
        if len(self.processors) > 1:
            busy = self.tx_state()["pendingModulation"]
            if (busy if m is None else busy & m).any():
                raise RuntimeError("Modulation already in progress")  # fsk-processor.ts:91
        self._fan_out(lambda i, p, first, count: p.modulate(rows[first:first + count], None if m is None else m[first:first + count]))

    def tx_state(self):
        parts = self._fan_out(lambda i, p, first, count: p.tx_state())
        return {k: np.concatenate([np.asarray(t[k]) for t in parts]) for k in parts[0]} if parts else {}

    def demodulate(self):
        return [b for part in self._fan_out(lambda i, p, first, count: p.demodulate()) for b in part]

    def demodulate_sparse(self, mask=None, min_len=1):
        """FSKProcessorBatch.demodulate_sparse over the shards: (streams, offsets, data) with GLOBAL stream numbers, ascending, and
        one CSR over all of them."""
        m = None
        if mask is not None:
            m = np.asarray(mask, dtype=bool).reshape(-1)
            if len(m) != self.n_streams:
                raise ValueError("mask must have one entry per stream")
        parts = self._fan_out(lambda i, p, first, count: p.demodulate_sparse(mask=None if m is None else m[first:first + count], min_len=min_len))
        streams, offsets, data, at = [], [np.zeros(1, np.uint32)], [], 0
        for (first, _count, _dev), (s, o, d) in zip(self.shards, parts):
            streams.append(np.asarray(s, np.uint32) + np.uint32(first))
            offsets.append(np.asarray(o[1:], np.uint32) + np.uint32(at))
            data.append(np.asarray(d, np.uint8))
            at += len(d)
        return np.concatenate(streams) if streams else np.zeros(0, np.uint32), np.concatenate(offsets), np.concatenate(data) if data else np.zeros(0, np.uint8)

    def demodulate_active(self, mask=None, min_len=1):
        """demodulate_sparse as {global stream: bytes} of the streams that held any."""
        streams, offsets, data = self.demodulate_sparse(mask=mask, min_len=min_len)
        return {int(s): data[offsets[i]:offsets[i + 1]].tobytes() for i, s in enumerate(streams)}

    def rx_lengths(self):
        parts = self._fan_out(lambda i, p, first, count: p.rx_lengths())
        return np.concatenate([np.asarray(x, np.uint32) for x in parts]) if parts else np.zeros(0, np.uint32)

    def reset(self, stream=-1):
        if stream < 0:
            self._fan_out(lambda i, p, first, count: p.reset(-1))
        else:
            i, local = self.locate(stream)
            self.processors[i].reset(local)

    def status(self, stream=0):
        """The 'status' reply for one (global) stream; processDemodulationCallCount is the batch's."""
        i, local = self.locate(stream)
        st = self.processors[i].status(local)
        st["processDemodulationCallCount"] = self.processDemodulationCallCount
        return st
