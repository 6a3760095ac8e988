'use strict';
// FSKProcessorBatch: S instances of the reference's FSKProcessor (src/webaudio/processors/fsk-processor.ts) on one
// GPU.  process(inputs, nOut) is process() for every stream in one call: demodulated bytes go into per-stream RX
// rings on the device, pending modulations are fed from the device; modulate / demodulate / reset / status mirror
// the worklet's message handlers (without the waiting: callers poll).  remap / snapshot / fromSnapshot carry the rings and
// pending modulations along with the batch's streams (FSKBatch.remap / snapshot / fromSnapshot underneath).
const path = require('path');
const addon = require(path.join(__dirname, 'fsk_addon.node'));
const { FSKBatch, sampleFormat, sampleLayout } = require(path.join(__dirname, 'fsk-core.js'));
const { Upsampler, Downsampler, CaptureConverter, PlaybackConverter } = require(path.join(__dirname, 'filters.js'));
const { busyError } = require(path.join(__dirname, 'errors.js'));
const PROC_CLEAR_RX_ON_TX_COMPLETE = 1, PROC_GRAPH = 2, PROC_RATECVT_PAIR = 4;

class FSKProcessorBatch {
  // batch: an FSKBatch (fsk-core.js); rxCapacity 1024 = demodulatedBuffer (fsk-processor.ts:84)
  constructor(batch, options = {}) {
    this.batch = batch;
    this.nStreams = batch.nStreams;
    this.rxCapacity = options.rxCapacity || 1024;
    this.flags = (options.clearRxOnTxComplete === false ? 0 : PROC_CLEAR_RX_ON_TX_COMPLETE) | (options.useGraph ? PROC_GRAPH : 0);
    this.handle = addon.processorCreate(batch.handle, this.rxCapacity);
    this.processDemodulationCallCount = 0;
  }
  close() { if (this.handle) { addon.processorDestroy(this.handle); this.handle = null; } }

  _options() {
    return { rxCapacity: this.rxCapacity, clearRxOnTxComplete: !!(this.flags & PROC_CLEAR_RX_ON_TX_COMPLETE), useGraph: !!(this.flags & PROC_GRAPH) };
  }
  // a new FSKProcessorBatch of map.length streams whose stream i continues stream map[i] of this one -- its FSKCore (FSKBatch.remap)
  // and its FSKProcessor: ring, pending modulation, completed count -- or starts as a new one where map[i] is -1.  The new
  // processor batch owns its FSKBatch (close both); this one is left as it is.  processDemodulationCallCount is carried.
  remap(map, configs) {
    const m = Array.from(map, Number);
    const batch = this.batch.remap(m, configs);
    let next = null;
    try {
      next = new FSKProcessorBatch(batch, this._options());
      addon.processorRemap(next.handle, this.handle, m);
    } catch (err) {
      if (next) next.close();
      batch.close();
      throw err;
    }
    next.processDemodulationCallCount = this.processDemodulationCallCount;
    return next;
  }
  // {engine, processor}: the FSKBatch's snapshot and the processors' own image, two Buffers taken at one moment
  snapshot(streams) {
    const sel = streams === undefined || streams === null ? null : Array.from(streams, Number);
    return { engine: this.batch.snapshot(sel), processor: addon.processorSnapshot(this.handle, sel) };
  }
  // a new FSKProcessorBatch whose stream i continues RECORD map[i] of both images (-1: a new stream; undefined: every record in
  // order).  options: useGraph, clearRxOnTxComplete; rxCapacity is the image's.  processDemodulationCallCount starts at 0.
  static fromSnapshot(snap, map, configs, device, options = {}) {
    const info = addon.processorSnapshotInfo(snap.processor);
    const m = map === undefined || map === null ? Array.from({ length: info.nStreams }, (_, i) => i) : Array.from(map, Number);
    const batch = FSKBatch.fromSnapshot(snap.engine, m, configs, device);
    let next = null;
    try {
      next = new FSKProcessorBatch(batch, Object.assign({}, options, { rxCapacity: info.rxCapacity }));
      addon.processorRestore(next.handle, snap.processor, m);
    } catch (err) {
      if (next) next.close();
      batch.close();
      throw err;
    }
    return next;
  }

  // process(inputs, outputs) fsk-processor.ts:152-167.  inputs: Float32Array [S][nIn] or null; returns Float32Array [S][nOut] or null
  // out (optional): the Float32Array [S][nOut] to write and return instead of a new one
  process(inputs, nIn, nOut, out) {
    if (inputs) this.processDemodulationCallCount++;
    return addon.processorProcess(this.handle, inputs || null, inputs ? nIn : 0, inputs ? nIn : 0, nOut || 0, this.flags, out || null);
  }
  // process() with either side in a capture format and layout (fskhip_processor_process_fmt_host): inputs is the input format's typed
  // array -- Float32Array 'f32', Int16Array 's16', Uint8Array 'mulaw' / 'alaw' -- or null, input = {format, layout, nIn, pitch},
  // output = {format, layout, nOut, pitch}; layout 'stream' = [S][pitch >= n], 'sample' = interleaved frames [n][pitch >= S]; format
  // defaults to 'f32', layout to 'stream', pitch to the packed one.  Returns the output format's typed array, or null when nOut is 0.
  // The samples cross PCIe as they are; state and output are those of process() on the decoded floats, the output encoded.
  // output.out (optional, in the rate forms as well): the typed array of the output format to write and return instead of a new
  // one -- at output.pitch it may be a view into a wider array, a shard's column block of interleaved frames.
  processSamples(inputs, input = {}, output = {}) {
    if (input === null || typeof input !== 'object' || output === null || typeof output !== 'object') {
      throw new TypeError('processSamples: input and output must be objects {format, layout, nIn | nOut, pitch}');
    }
    const inFmt = sampleFormat(input.format === undefined ? 'f32' : input.format), inLay = sampleLayout(input.layout);
    const outFmt = sampleFormat(output.format === undefined ? 'f32' : output.format), outLay = sampleLayout(output.layout);
    const count = (v, what) => {
      const n = v === undefined ? 0 : v;
      if (!Number.isInteger(n) || n < 0 || n > 0xffffffff) throw new RangeError('processSamples: ' + what + ' must be an integer in [0, 2^32)');
      return n;
    };
    const has = inputs !== undefined && inputs !== null;
    if (has && !ArrayBuffer.isView(inputs)) throw new TypeError('processSamples: inputs must be a typed array or null');
    const nIn = has ? count(input.nIn, 'nIn') : 0, nOut = count(output.nOut, 'nOut');
    const inPitch = count(input.pitch, 'input pitch') || (inLay ? this.nStreams : nIn);
    const outPitch = count(output.pitch, 'output pitch') || (outLay ? this.nStreams : nOut);
    if (has) this.processDemodulationCallCount++;      // (as process() counts: behind the argument checks, in front of the call)
    return addon.processorProcessSamples(this.handle, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags, output.out || null);
  }
  // processSamples() with both sides at the trunk's own rate (fskhip_processor_process_rate_host): input = {format, layout, nIn, pitch,
  // upsampler}, output = {format, layout, nOut, pitch, downsampler} with the Upsampler / Downsampler of filters.js, which interpolate
  // the inputs in front of the demodulator and decimate the pending modulation on the device; lengths and pitches count low rate
  // elements, format defaults to 'mulaw' and layout to 'sample' (interleaved frames).  Both handles carry their histories from call
  // to call; state and samples are those of Upsampler.process -> process() -> Downsampler.process, bit for bit.  A side without
  // samples needs no handle.  With a CaptureConverter as upsampler and a PlaybackConverter as downsampler both sides are at the
  // converters' outer rate (44.1 kHz either side of a 48 kHz engine; fskhip_processor_process_ratecvt_host): nIn a multiple of the
  // capture converter's down, nOut of the playback converter's up; one call takes resamplers or converters, not one of each.
  processSamplesAt(inputs, input = {}, output = {}) { return this.samplesAt('processSamplesAt', false, inputs, input, output); }
  // processSamplesAt() through a CaptureConverter and a PlaybackConverter for quanta of any length -- a 128-frame render quantum at
  // 44.1 kHz as it arrives (fskhip_processor_process_ratecvt_any_host): the handles carry their positions from call to call; state
  // and samples are those of processAny -> process() with the engine counts the handles give -> processAny, bit for bit.  A
  // resampler in a slot is a TypeError; an nOut the playback converter cannot write from its position is the library's refusal.
  processSamplesAtAny(inputs, input = {}, output = {}) { return this.samplesAt('processSamplesAtAny', true, inputs, input, output); }
  samplesAt(who, anyLength, inputs, input, output) {
    if (input === null || typeof input !== 'object' || output === null || typeof output !== 'object') {
      throw new TypeError(who + ': input and output must be objects {format, layout, nIn | nOut, pitch, upsampler | downsampler}');
    }
    const inFmt = sampleFormat(input.format === undefined ? 'mulaw' : input.format), inLay = sampleLayout(input.layout === undefined ? 'sample' : input.layout);
    const outFmt = sampleFormat(output.format === undefined ? 'mulaw' : output.format), outLay = sampleLayout(output.layout === undefined ? 'sample' : output.layout);
    const count = (v, what) => {
      const n = v === undefined ? 0 : v;
      if (!Number.isInteger(n) || n < 0 || n > 0xffffffff) throw new RangeError(who + ': ' + what + ' must be an integer in [0, 2^32)');
      return n;
    };
    const has = inputs !== undefined && inputs !== null;
    if (has && !ArrayBuffer.isView(inputs)) throw new TypeError(who + ': inputs must be a typed array or null');
    const nIn = has ? count(input.nIn, 'nIn') : 0, nOut = count(output.nOut, 'nOut');
    const inPitch = count(input.pitch, 'input pitch') || (inLay ? this.nStreams : nIn);
    const outPitch = count(output.pitch, 'output pitch') || (outLay ? this.nStreams : nOut);
    const handle = (r, kind, converter, what) => {     // (a converter of the side's direction stands in its resampler's place)
      if (!(r instanceof kind) && !(r instanceof converter)) throw new TypeError(who + ': ' + what + ' must be an ' + kind.name + ' of filters.js');
      if (r.nStreams !== this.nStreams) throw new RangeError(who + ': ' + what + ' has ' + r.nStreams + ' streams, the batch ' + this.nStreams);
      return r.handle;
    };
    const up = has ? handle(input.upsampler, Upsampler, CaptureConverter, 'upsampler') : null;
    const down = nOut ? handle(output.downsampler, Downsampler, PlaybackConverter, 'downsampler') : null;
    // converters: both sides at their outer rate (fskhip_processor_process_ratecvt_host), in whole periods; one call takes one kind
    const capture = has && input.upsampler instanceof CaptureConverter, playback = nOut > 0 && output.downsampler instanceof PlaybackConverter;
    if (has && nOut && capture !== playback) {
      throw new TypeError(who + ': upsampler is a ' + input.upsampler.constructor.name + ' and downsampler a ' + output.downsampler.constructor.name +
        ': one call takes resamplers or rate converters, not one of each');
    }
    if (anyLength) {
      if (has && !capture) throw new TypeError(who + ': upsampler is a ' + input.upsampler.constructor.name + ': quanta of any length go through rate converters');
      if (nOut && !playback) throw new TypeError(who + ': downsampler is a ' + output.downsampler.constructor.name + ': quanta of any length go through rate converters');
      if (has) this.processDemodulationCallCount++;
      return addon.processorProcessSamplesAtAny(this.handle, up, down, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags, output.out || null);
    }
    if (capture && nIn % input.upsampler.down) {
      throw new RangeError(who + ': ' + nIn + ' samples per stream are not a multiple of the converter\'s down factor ' + input.upsampler.down);
    }
    if (playback && nOut % output.downsampler.up) {
      throw new RangeError(who + ': nOut ' + nOut + ' is not a multiple of the converter\'s up factor ' + output.downsampler.up);
    }
    if (has) this.processDemodulationCallCount++;      // (as process() counts: behind the argument checks, in front of the call)
    return addon.processorProcessSamplesAt(this.handle, up, down, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags, output.out || null);
  }
  // 'modulate' (87-113): payloads = array of S Uint8Array; mask = optional array of S booleans
  modulate(payloads, mask) {
    let mx = 1;
    for (const p of payloads) mx = Math.max(mx, p.length);
    const slab = new Uint8Array(mx * this.nStreams);
    const lens = new Uint32Array(this.nStreams);
    payloads.forEach((p, i) => { slab.set(p, i * mx); lens[i] = p.length; });
    try {
      addon.processorModulate(this.handle, slab, lens, mx, mask ? Uint8Array.from(mask.map((b) => (b ? 1 : 0))) : null);
    } catch (e) {
      throw busyError(e, 'Modulation already in progress');   // fsk-processor.ts:91
    }
  }
  txState() { return addon.processorTxState(this.handle); }
  // fskhip_processor_last_tx_kernel: the kernel that wrote the last quantum's output, or the two launches that stand for one joined
  // by '+' ('processor_io_ratecvt_kernel<any>', 'processor_io_kernel+ratecvt_playback_any_kernel', ...); '' where it had no TX side
  get lastTxKernel() { return addon.processorLastTxKernel(this.handle); }
  // 'demodulate' (117-138) without the wait: everything buffered, per stream
  demodulate() {
    const r = addon.processorDrain(this.handle, this.rxCapacity);
    const out = [];
    for (let s = 0; s < this.nStreams; s++) out.push(r.out.slice(s * r.outPitch, s * r.outPitch + r.counts[s]));
    return out;
  }
  // the same for the streams that hold bytes only: {streams, offsets, data} -- the streams with at least max(minLen, 1) buffered
  // bytes (and mask[s], where a mask is given) in ascending order; the bytes of streams[i] are data.subarray(offsets[i], offsets[i + 1]).
  // Streams not listed keep their rings.
  rxDrainSparse(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('rxDrainSparse: options must be an object {mask, minLen}');
    const { mask, minLen = 1 } = options;
    if (!Number.isInteger(minLen) || minLen < 0 || minLen > 0xffffffff) throw new RangeError('rxDrainSparse: minLen must be an integer in [0, 2^32)');
    let m = null;
    if (mask !== undefined && mask !== null) {
      if (!Array.isArray(mask) && !ArrayBuffer.isView(mask)) throw new TypeError('rxDrainSparse: mask must be an array of nStreams booleans');
      if (mask.length !== this.nStreams) throw new RangeError('rxDrainSparse: mask must have one entry per stream (' + this.nStreams + ')');
      m = Uint8Array.from(mask, (b) => (b ? 1 : 0));
    }
    return addon.processorDrainSparse(this.handle, m, minLen);
  }
  rxLengths() { return addon.processorRxLength(this.handle); }
  reset(stream = -1) { addon.processorReset(this.handle, stream); }
  status(stream = 0) {               // the 'status' reply (240-253)
    const tx = this.txState();
    return Object.assign({ demodulatedBufferLength: this.rxLengths()[stream], pendingModulation: !!tx.pending[stream],
      fskCoreReady: true, processDemodulationCallCount: this.processDemodulationCallCount }, this.batch.getStatus(stream));
  }
}
// FSKProcessorBatchSharded: S FSKProcessors over several GPUs -- one FSKBatch and one FSKProcessorBatch per device over contiguous
// blocks of streams, as FSKBatchSharded (fsk-core.js) shards the engine.  The methods are FSKProcessorBatch's over the host forms,
// stream indices are global, and a quantum costs no host copy: a shard reads its row block of a stream-major array, or its column
// block of interleaved frames at the full frame pitch, and writes its block of ONE output array.  The rate forms take arrays of
// handles, one per shard.  remap / snapshot / fromSnapshot move live processors between devices through one pair of images
// (snapshotConcat, processorSnapshotConcat).  options: devices (default [0]), precision, rxCapacity, clearRxOnTxComplete, useGraph.
const ARRAY_OF = [Float32Array, Int16Array, Uint8Array, Uint8Array];
class FSKProcessorBatchSharded {
  constructor(nStreams, configs, options = {}) {
    this.nStreams = nStreams;
    this.options = Object.assign({}, options);
    this.processDemodulationCallCount = 0;
    this.shards = [];
    if (options._shards) { this.shards = options._shards; delete this.options._shards; return; }
    if (Array.isArray(configs) && configs.length !== nStreams) throw new Error('need one config per stream');
    try {
      FSKProcessorBatchSharded.blocks(nStreams, options.devices || [0]).forEach((sh) => {
        const cfg = Array.isArray(configs) ? configs.slice(sh.first, sh.first + sh.count) : configs;
        const batch = new FSKBatch(sh.count, cfg, { device: sh.device, precision: options.precision });
        let procs = null;
        try { procs = new FSKProcessorBatch(batch, options); } catch (e) { batch.close(); throw e; }
        this.shards.push(Object.assign(sh, { batch, procs }));
      });
    } catch (e) {
      this.close();
      throw e;
    }
  }
  // the shard table: contiguous blocks, the first nStreams % devices.length one stream longer; devices with nothing to do left out
  static blocks(nStreams, devices) {
    if (!devices.length) throw new Error('no devices');
    const base = Math.floor(nStreams / devices.length), extra = nStreams % devices.length, out = [];
    let first = 0;
    devices.forEach((device, r) => {
      const count = base + (r < extra ? 1 : 0);
      if (count > 0) out.push({ first, count, device });
      first += count;
    });
    return out;
  }
  get processors() { return this.shards.map((sh) => sh.procs); }
  get batches() { return this.shards.map((sh) => sh.batch); }
  get rxCapacity() { return this.shards.length ? this.shards[0].procs.rxCapacity : (this.options.rxCapacity || 1024); }
  locate(stream) {
    for (const sh of this.shards) if (stream >= sh.first && stream < sh.first + sh.count) return [sh, stream - sh.first];
    throw new Error('stream out of range');
  }
  close() { this.shards.forEach((sh) => { sh.procs.close(); sh.batch.close(); }); this.shards = []; }

  process(inputs, nIn, nOut, out) {
    const n = nOut || 0;
    const o = n ? (out || new Float32Array(n * this.nStreams)) : null;
    if (o && o.length < n * this.nStreams) throw new RangeError('out too short');
    for (const sh of this.shards) {
      sh.procs.process(inputs ? inputs.subarray(sh.first * nIn, (sh.first + sh.count) * nIn) : null, nIn, n, o ? o.subarray(sh.first * n, (sh.first + sh.count) * n) : null);
    }
    if (inputs) this.processDemodulationCallCount++;
    return o;
  }
  // the whole-batch geometry of a format quantum, and per shard the views and option objects of its block
  _plan(who, inputs, input, output, defFmt, defLay) {
    if (input === null || typeof input !== 'object' || output === null || typeof output !== 'object') throw new TypeError(who + ': input and output must be objects');
    const inLay = sampleLayout(input.layout === undefined ? defLay : input.layout), outLay = sampleLayout(output.layout === undefined ? defLay : output.layout);
    const inFmt = sampleFormat(input.format === undefined ? defFmt : input.format), outFmt = sampleFormat(output.format === undefined ? defFmt : output.format);
    const has = inputs !== undefined && inputs !== null;
    const nIn = has ? (input.nIn || 0) : 0, nOut = output.nOut || 0;
    const inPitch = input.pitch || (inLay ? this.nStreams : nIn), outPitch = output.pitch || (outLay ? this.nStreams : nOut);
    let out = null;
    if (nOut) {
      const rows = outLay ? nOut : this.nStreams, cols = outLay ? this.nStreams : nOut;
      if (outPitch < cols) throw new RangeError(who + ': output pitch too small');
      const need = outPitch * (rows - 1) + cols;
      out = output.out;
      if (out === undefined || out === null) {
        out = new ARRAY_OF[outFmt](need);
        if (outFmt >= 2) out.fill(outFmt === 2 ? 0xff : 0xd5);   // (the pitch's padding: silence, like the rest)
      }
      if (!(out instanceof ARRAY_OF[outFmt]) || out.length < need) throw new RangeError(who + ': out must be a ' + ARRAY_OF[outFmt].name + ' of at least ' + need + ' elements');
    }
    const view = (a, lay, n, pitch, sh) => (lay ? a.subarray(sh.first, pitch * (n - 1) + sh.first + sh.count) : a.subarray(sh.first * pitch, (sh.first + sh.count - 1) * pitch + n));
    const calls = this.shards.map((sh) => ({
      procs: sh.procs,
      inputs: has && nIn ? view(inputs, inLay, nIn, inPitch, sh) : (has ? inputs : null),
      input: Object.assign({}, input, { format: inFmt, layout: inLay, nIn, pitch: inPitch }),
      output: Object.assign({}, output, { format: outFmt, layout: outLay, nOut, pitch: outPitch, out: out ? view(out, outLay, nOut, outPitch, sh) : null }),
    }));
    return { has, nIn, nOut, out, calls };
  }
  processSamples(inputs, input = {}, output = {}) {
    const p = this._plan('processSamples', inputs, input, output, 'f32', 'stream');
    p.calls.forEach((c) => c.procs.processSamples(c.inputs, c.input, c.output));
    if (p.has) this.processDemodulationCallCount++;
    return p.out;
  }
  // the rate forms: input.upsampler / output.downsampler are ARRAYS of handles, one per shard, each of its shard's stream count and
  // on its device.  A wrong count of handles or stream count is refused before any shard is called, so no state moves; quanta of
  // any length want every handle of a side at the same position.
  _samplesAt(who, anyLength, inputs, input, output) {
    const p = this._plan(who, inputs, input, output, 'mulaw', 'sample');
    const side = (handles, wanted, what) => {
      if (!wanted) return this.shards.map(() => undefined);
      if (!Array.isArray(handles) || handles.length !== this.shards.length) throw new RangeError(who + ': ' + what + ' must be an array of ' + this.shards.length + ' handles, one per shard');
      handles.forEach((h, i) => {
        if (!h || h.nStreams !== this.shards[i].count) throw new RangeError(who + ': ' + what + ' ' + i + ' has ' + (h && h.nStreams) + ' streams, its shard ' + this.shards[i].count);
        if (h.device !== undefined && h.device !== this.shards[i].device) throw new RangeError(who + ': ' + what + ' ' + i + ' is on device ' + h.device + ', its shard on ' + this.shards[i].device);
      });
      if (anyLength && new Set(handles.map((h) => h.position)).size > 1) throw new RangeError(who + ': the ' + what + ' handles stand at different positions');
      return handles;
    };
    const ups = side(input.upsampler, p.has, 'upsampler'), downs = side(output.downsampler, p.nOut > 0, 'downsampler');
    p.calls.forEach((c, i) => {      // every shard's argument checks (the single class's) before any shard is called
      c.input.upsampler = ups[i]; c.output.downsampler = downs[i];
    });
    p.calls.forEach((c) => c.procs.samplesAt(who, anyLength, c.inputs, c.input, c.output));
    if (p.has) this.processDemodulationCallCount++;
    return p.out;
  }
  processSamplesAt(inputs, input = {}, output = {}) { return this._samplesAt('processSamplesAt', false, inputs, input, output); }
  processSamplesAtAny(inputs, input = {}, output = {}) { return this._samplesAt('processSamplesAtAny', true, inputs, input, output); }
  get lastTxKernel() { return this.shards.map((sh) => sh.procs.lastTxKernel); }

  // as FSKProcessorBatch.modulate, a masked stream with a modulation pending refuses the whole call and nothing starts on any
  // shard: the shards are asked first (the refusal's text is this wrapper's)
  modulate(payloads, mask) {
    if (payloads.length !== this.nStreams) throw new Error('need one payload per stream');
    if (mask && mask.length !== this.nStreams) throw new RangeError('mask must have one entry per stream');
    const pending = this.txState().pending;
    for (let s = 0; s < this.nStreams; s++) if (pending[s] && (!mask || mask[s])) throw new Error('Modulation already in progress');
    for (const sh of this.shards) sh.procs.modulate(payloads.slice(sh.first, sh.first + sh.count), mask ? Array.from(mask).slice(sh.first, sh.first + sh.count) : undefined);
  }
  txState() {
    const out = { pos: new Uint32Array(this.nStreams), total: new Uint32Array(this.nStreams), pending: new Uint8Array(this.nStreams), completed: new Uint32Array(this.nStreams) };
    for (const sh of this.shards) { const t = sh.procs.txState(); for (const k of Object.keys(out)) out[k].set(t[k], sh.first); }
    return out;
  }
  demodulate() { let out = []; for (const sh of this.shards) out = out.concat(sh.procs.demodulate()); return out; }
  // {streams, offsets, data} with GLOBAL stream numbers, ascending, and one CSR over all shards
  rxDrainSparse(options = {}) {
    if (options === null || typeof options !== 'object') throw new TypeError('rxDrainSparse: options must be an object {mask, minLen}');
    const { mask, minLen = 1 } = options;
    if (mask !== undefined && mask !== null && mask.length !== this.nStreams) throw new RangeError('rxDrainSparse: mask must have one entry per stream (' + this.nStreams + ')');
    const parts = this.shards.map((sh) => sh.procs.rxDrainSparse({ mask: mask ? Array.from(mask).slice(sh.first, sh.first + sh.count) : undefined, minLen }));
    let ns = 0, nb = 0;
    parts.forEach((r) => { ns += r.streams.length; nb += r.data.length; });
    const streams = new Uint32Array(ns), offsets = new Uint32Array(ns + 1), data = new Uint8Array(nb);
    let si = 0, bi = 0;
    parts.forEach((r, k) => {
      for (let i = 0; i < r.streams.length; i++) { streams[si + i] = r.streams[i] + this.shards[k].first; offsets[si + i + 1] = bi + r.offsets[i + 1]; }
      data.set(r.data.subarray(0, r.offsets[r.streams.length]), bi);
      si += r.streams.length; bi += r.offsets[r.streams.length];
    });
    return { streams, offsets, data: data.subarray(0, bi) };
  }
  rxLengths() {
    const out = new Uint32Array(this.nStreams);
    for (const sh of this.shards) out.set(sh.procs.rxLengths(), sh.first);
    return out;
  }
  reset(stream = -1) {
    if (stream < 0) this.shards.forEach((sh) => sh.procs.reset());
    else { const [sh, local] = this.locate(stream); sh.procs.reset(local); }
  }
  status(stream = 0) {
    const [sh, local] = this.locate(stream);
    return Object.assign(sh.procs.status(local), { processDemodulationCallCount: this.processDemodulationCallCount });
  }
  // {engine, processor} of the whole batch, records in global stream order: the shards' pairs under one header each
  snapshot() {
    const parts = this.shards.map((sh) => sh.procs.snapshot());
    if (parts.length === 1) return parts[0];
    return { engine: addon.snapshotConcat(parts.map((s) => s.engine)), processor: addon.processorSnapshotConcat(parts.map((s) => s.processor)) };
  }
  // a new sharded batch whose stream i continues RECORD map[i] of a snapshot() pair (a sharded batch's or a single
  // FSKProcessorBatch's; -1: a new stream; undefined: every record in order) over options.devices: every shard restores its
  // slice of the map.  processDemodulationCallCount starts at 0.
  static fromSnapshot(snap, map, configs, options = {}) {
    const info = addon.processorSnapshotInfo(snap.processor);
    const m = map === undefined || map === null ? Array.from({ length: info.nStreams }, (_, i) => i) : Array.from(map, Number);
    const shards = [];
    try {
      FSKProcessorBatchSharded.blocks(m.length, options.devices || [0]).forEach((sh) => {
        const cfg = Array.isArray(configs) ? configs.slice(sh.first, sh.first + sh.count) : configs;
        const procs = FSKProcessorBatch.fromSnapshot(snap, m.slice(sh.first, sh.first + sh.count), cfg, sh.device, options);
        shards.push(Object.assign(sh, { batch: procs.batch, procs }));
      });
    } catch (e) {
      shards.forEach((sh) => { sh.procs.close(); sh.batch.close(); });
      throw e;
    }
    return new FSKProcessorBatchSharded(m.length, configs, Object.assign({}, options, { rxCapacity: info.rxCapacity, _shards: shards }));
  }
  // a new sharded batch of map.length streams whose stream i continues GLOBAL stream map[i] of this one (-1: a new one), across
  // shards and devices (options.devices, default: this batch's).  This batch is left as it is.  The call count is carried.
  remap(map, configs, options = {}) {
    const devices = options.devices || this.shards.map((sh) => sh.device);
    const next = FSKProcessorBatchSharded.fromSnapshot(this.snapshot(), map, configs, Object.assign({}, this.options, options, { devices }));
    next.processDemodulationCallCount = this.processDemodulationCallCount;
    next.shards.forEach((sh) => { sh.procs.processDemodulationCallCount = this.processDemodulationCallCount; });
    return next;
  }
}
const processorSnapshotInfo = (buf) => addon.processorSnapshotInfo(buf);
// fskhip_processor_snapshot_concat: one processor image holding the records of `bufs` in order, in canonical form -- byte for byte
// the image one FSKProcessorBatch holding the same streams writes (host only).  With snapshotConcat (fsk-core.js) for the engines'
// images it puts the pairs of one FSKProcessorBatch per GPU under one pair, which fromSnapshot restores slice by slice.
const processorSnapshotConcat = (bufs) => addon.processorSnapshotConcat(bufs);
module.exports = { FSKProcessorBatch, FSKProcessorBatchSharded, processorSnapshotInfo, processorSnapshotConcat, PROC_CLEAR_RX_ON_TX_COMPLETE, PROC_GRAPH, PROC_RATECVT_PAIR };
