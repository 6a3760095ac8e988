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
  process(inputs, nIn, nOut) {
    if (inputs) this.processDemodulationCallCount++;
    return addon.processorProcess(this.handle, inputs || null, inputs ? nIn : 0, inputs ? nIn : 0, nOut || 0, this.flags);
  }
  // process() with either side in a capture format and layout (fskhip_processor_process_fmt_host): inputs is the input format's typed
  // array -- Float32Array 'f32', Int16Array 's16', Uint8Array 'mulaw' / 'alaw' -- or null, input = {format, layout, nIn, pitch},
  // output = {format, layout, nOut, pitch}; layout 'stream' = [S][pitch >= n], 'sample' = interleaved frames [n][pitch >= S]; format
  // defaults to 'f32', layout to 'stream', pitch to the packed one.  Returns the output format's typed array, or null when nOut is 0.
  // The samples cross PCIe as they are; state and output are those of process() on the decoded floats, the output encoded.
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
    return addon.processorProcessSamples(this.handle, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags);
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
      return addon.processorProcessSamplesAtAny(this.handle, up, down, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags);
    }
    if (capture && nIn % input.upsampler.down) {
      throw new RangeError(who + ': ' + nIn + ' samples per stream are not a multiple of the converter\'s down factor ' + input.upsampler.down);
    }
    if (playback && nOut % output.downsampler.up) {
      throw new RangeError(who + ': nOut ' + nOut + ' is not a multiple of the converter\'s up factor ' + output.downsampler.up);
    }
    if (has) this.processDemodulationCallCount++;      // (as process() counts: behind the argument checks, in front of the call)
    return addon.processorProcessSamplesAt(this.handle, up, down, has ? inputs : null, inFmt, inLay, nIn, inPitch, outFmt, outLay, nOut, outPitch, this.flags);
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
const processorSnapshotInfo = (buf) => addon.processorSnapshotInfo(buf);
module.exports = { FSKProcessorBatch, processorSnapshotInfo, PROC_CLEAR_RX_ON_TX_COMPLETE, PROC_GRAPH, PROC_RATECVT_PAIR };
