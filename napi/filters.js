'use strict';
// src/dsp/filters.ts with the reference's names: FilterDesign.butterworth* / sinc*, IIRFilter, FIRFilter, FilterFactory.createIIR* /
// createFIR*, plus IIRFilterBatch / FIRFilterBatch (S streams per call).  Designs and filtering run in libfskhip.so.
const path = require('path');
const addon = require(path.join(__dirname, 'fsk_addon.node'));
const PRECISION_F32 = 0, PRECISION_F64 = 1;

function bw(kind, f, bandwidth, sampleRate) {
  const c = addon.butterworth(kind, f, bandwidth, sampleRate);
  return { b: [c[0], c[1], c[2]], a: [c[3], c[4], c[5]] };
}
class FilterDesign {
  static butterworthLowpass(cutoffFreq, sampleRate) { return bw(0, cutoffFreq, 0, sampleRate); }          // filters.ts:180-192
  static butterworthHighpass(cutoffFreq, sampleRate) { return bw(1, cutoffFreq, 0, sampleRate); }         // filters.ts:200-212
  static butterworthBandpass(centerFreq, bandwidth, sampleRate) { return bw(2, centerFreq, bandwidth, sampleRate); }   // filters.ts:221-234
  static sincLowpass(cutoffFreq, sampleRate, numTaps) { return Array.from(addon.sincLowpass(cutoffFreq, sampleRate, numTaps)); }
  static sincHighpass(cutoffFreq, sampleRate, numTaps) { return Array.from(addon.sincHighpass(cutoffFreq, sampleRate, numTaps)); }
  static sincBandpass(centerFreq, bandwidth, sampleRate, numTaps) { return Array.from(addon.sincBandpass(centerFreq, bandwidth, sampleRate, numTaps)); }
}

// [nStreams][n] in one typed array: n, or an error for a length that is not a whole number of samples per stream
function samplesPerStream(input, nStreams) {
  if (input.length % nStreams !== 0) throw new RangeError('input length ' + input.length + ' is not a multiple of the stream count ' + nStreams);
  return input.length / nStreams;
}

class FIRFilterBatch {
  constructor(coefficients, nStreams = 1, options = {}) {
    this.coefficients = [...coefficients];
    this.nStreams = nStreams;
    this.handle = addon.firCreate(Float64Array.from(coefficients), nStreams, options.device || 0,
      options.precision === undefined ? PRECISION_F64 : options.precision);
  }
  // input: Float32Array [nStreams][n]
  processBuffer(input) {
    const n = samplesPerStream(input, this.nStreams);
    if (n === 0) return new Float32Array(0);
    return addon.firProcess(this.handle, input, n, n, this.nStreams);
  }
  reset(stream = -1) { addon.firReset(this.handle, stream); }
  getCoefficients() { return [...this.coefficients]; }
  close() { if (this.handle) { addon.firDestroy(this.handle); this.handle = null; } }
}

class FIRFilter extends FIRFilterBatch {          // filters.ts:112-167
  constructor(coefficients, options = {}) { super(coefficients, 1, options); }
  process(input) { return this.processBuffer(Float32Array.of(input))[0]; }
}

// Rate conversion by an integer factor on the GPU (include/fskhip_next.h: fskhip_resampler_*): capture samples at lowRate <-> float32
// [nStreams][n] at factor * lowRate, the history carried across calls.  Without taps the design is sincLowpass(0.45 * lowRate,
// factor * lowRate, 16 * factor + 1) -- times factor in the up direction --: 97 taps and 3 600 Hz for 8 kHz <-> 48 kHz.
const SAMPLE_FORMATS = { f32: 0, s16: 1, mulaw: 2, alaw: 3 };
const SAMPLE_TYPES = [Float32Array, Int16Array, Uint8Array, Uint8Array];
function sampleFormat(f) {
  const v = typeof f === 'string' ? SAMPLE_FORMATS[f.toLowerCase()] : f;
  if (!(v >= 0 && v <= 3)) throw new TypeError('unknown sample format ' + f);
  return v;
}
function sampleLayout(l) {
  const v = l === undefined || l === null ? 0 : typeof l === 'string' ? { stream: 0, sample: 1 }[l.toLowerCase()] : l;
  if (v !== 0 && v !== 1) throw new TypeError('unknown layout ' + l);
  return v;
}
// What the resamplers and the rate converters below share: a handle of the addon's UNIT family (resampler* / ratecvt*): reset, the
// history rows and close; and the two process calls' marshalling over an object `o` of either, `call` being the addon's function
// and last(n) its last argument (the factor, or the output count).
class RateHandle {
  reset(stream = -1) { addon[this.constructor.UNIT + 'Reset'](this.handle, stream); }
  state() { return addon[this.constructor.UNIT + 'State'](this.handle); }             // Float32Array [nStreams][history], oldest first
  setState(state) { addon[this.constructor.UNIT + 'SetState'](this.handle, state); }
  close() { if (this.handle) { addon[this.constructor.UNIT + 'Destroy'](this.handle); this.handle = null; } }
}
function rateWiden(o, call, samples, format, layout, nIn, pitch, last) {
  const f = sampleFormat(format), l = sampleLayout(layout);
  if (!(samples instanceof SAMPLE_TYPES[f])) throw new TypeError('format ' + format + ' takes a ' + SAMPLE_TYPES[f].name);
  const n = nIn === undefined ? samplesPerStream(samples, o.nStreams) : nIn;
  if (n === 0) return new Float32Array(0);
  return call(o.handle, samples, f, l, n, pitch === undefined ? (l === 1 ? o.nStreams : n) : pitch, last(n));
}
function rateNarrow(o, call, input, format, layout, lens, last) {
  const f = sampleFormat(format), l = sampleLayout(layout);
  const n = samplesPerStream(input, o.nStreams);
  if (n === 0) return new SAMPLE_TYPES[f](0);
  return call(o.handle, input, n, lens, f, l, last(n));
}
class Resampler extends RateHandle {
  static get UNIT() { return 'resampler'; }
  constructor(direction, factor, nStreams, options = {}) {
    super();
    if (!(Number.isInteger(factor) && factor >= 1 && factor <= 32)) throw new RangeError('factor ' + factor + ' outside 1..32');
    this.factor = factor;
    this.nStreams = nStreams;
    this.lowRate = options.lowRate === undefined ? 8000 : options.lowRate;
    let taps = options.taps;
    if (!taps) {
      taps = FilterDesign.sincLowpass(0.45 * this.lowRate, factor * this.lowRate, 16 * factor + 1);
      if (direction === 0) taps = taps.map((t) => t * factor);
    }
    this.taps = [...taps];
    this.handle = addon.resamplerCreate(direction, factor, Float64Array.from(this.taps), nStreams, options.device || 0,
      options.precision === undefined ? PRECISION_F32 : options.precision);
    this.history = addon.resamplerHistory(this.handle);
  }
  // an object of this class over a handle the library created (remap, restore)
  static adopt(handle, design) {
    const o = Object.create(this.prototype);
    o.factor = design.factor; o.lowRate = design.lowRate; o.taps = [...design.taps];
    o.handle = handle;
    o.nStreams = addon.resamplerStreams(handle);
    o.history = addon.resamplerHistory(handle);
    return o;
  }
  // fskhip_resampler_remap: a new object of this design whose stream i continues stream map[i] of this one (its history row, bit
  // for bit; -1: a zero history) -- the map the engine and the processor were remapped with.  This object stays usable.
  remap(map) { return this.constructor.adopt(addon.resamplerRemap(this.handle, Array.from(map)), this); }
  // fskhip_resampler_snapshot: the image of `streams` (null: all, in order) as a Buffer -- the design and the history rows
  snapshot(streams = null) { return addon.resamplerSnapshot(this.handle, streams === null || streams === undefined ? null : Array.from(streams)); }
  // fskhip_resampler_restore: a new object from a snapshot() alone; stream i continues record map[i] (-1: a zero history; null:
  // every record, in order).  Upsampler and Downsampler refuse an image of the other direction.
  static fromSnapshot(buf, map = null, options = {}) {
    const info = addon.resamplerSnapshotInfo(buf);
    if (this.DIRECTION !== undefined && info.direction !== this.DIRECTION) {
      throw new RangeError('the snapshot is of a resampler that goes ' + ['up', 'down'][info.direction] + ', not ' + ['up', 'down'][this.DIRECTION]);
    }
    const handle = addon.resamplerRestore(buf, map === null || map === undefined ? null : Array.from(map), options.device || 0);
    return this.adopt(handle, { factor: info.factor, lowRate: options.lowRate, taps: Array.from(info.taps) });
  }
}
function resamplerSnapshotInfo(buf) { return addon.resamplerSnapshotInfo(buf); }
class Upsampler extends Resampler {
  static get DIRECTION() { return 0; }
  constructor(factor, nStreams, options = {}) { super(0, factor, nStreams, options); }
  // samples: the format's typed array, [nStreams][pitch] (layout 'stream') or frames [nPerStream][pitch >= nStreams] ('sample');
  // nPerStream and pitch default to a packed array's -> Float32Array [nStreams][nPerStream * factor]
  process(samples, format, layout = 'stream', nPerStream, pitch) { return rateWiden(this, addon.resamplerUp, samples, format, layout, nPerStream, pitch, () => this.factor); }
}
class Downsampler extends Resampler {
  static get DIRECTION() { return 1; }
  constructor(factor, nStreams, options = {}) { super(1, factor, nStreams, options); }
  // input: Float32Array [nStreams][n], n a multiple of factor; lens (Uint32Array or null): stream s reads as 0.0 from lens[s] on
  // -> the format's typed array, [nStreams][n / factor] or frames [n / factor][nStreams]
  process(input, format, layout = 'stream', lens = null) { return rateNarrow(this, addon.resamplerDown, input, format, layout, lens, () => this.factor); }
}

// Rate conversion by a ratio up / down on the GPU (include/fskhip_next.h: fskhip_ratecvt_*): 44.1 kHz audio either side of a 48 kHz
// engine.  inRate -> outRate, the rates over their gcd (up and down each at most 256); a call takes a multiple of `down` samples
// per stream and gives n / down * up, the history carried across calls.  Without taps the design is sincLowpass(0.45 * min(inRate,
// outRate), up * inRate, 16 * max(up, down) + 1) times up: 2 561 taps and 19 845 Hz between 44.1 and 48 kHz.
function gcd(a, b) { while (b) { const t = a % b; a = b; b = t; } return a; }
class RateConverter extends RateHandle {
  static get UNIT() { return 'ratecvt'; }
  static ratio(inRate, outRate) {
    if (!(Number.isInteger(inRate) && Number.isInteger(outRate) && inRate >= 1 && outRate >= 1)) {
      throw new RangeError('rates must be positive whole numbers, got ' + inRate + ' and ' + outRate);
    }
    const g = gcd(inRate, outRate);
    return { up: outRate / g, down: inRate / g };
  }
  static defaultTaps(inRate, outRate) {
    const { up, down } = this.ratio(inRate, outRate), n = 16 * Math.max(up, down) + 1;
    if (n > 4096) throw new RangeError('the default design for ' + up + ' / ' + down + ' needs ' + n + ' taps, the limit is 4096');
    return FilterDesign.sincLowpass(0.45 * Math.min(inRate, outRate), up * inRate, n).map((t) => t * up);
  }
  constructor(direction, inRate, outRate, nStreams, options = {}) {
    super();
    const { up, down } = RateConverter.ratio(inRate, outRate);
    this.inRate = inRate; this.outRate = outRate; this.up = up; this.down = down;
    this.nStreams = nStreams;
    this.taps = [...(options.taps || RateConverter.defaultTaps(inRate, outRate))];
    this.handle = addon.ratecvtCreate(direction, up, down, Float64Array.from(this.taps), nStreams, options.device || 0,
      options.precision === undefined ? PRECISION_F32 : options.precision);
    this.history = addon.ratecvtHistory(this.handle);
  }
  outCount(nIn) { return Math.floor(nIn / this.down) * this.up; }
  // Calls of any length (fskhip_ratecvt_*_any_host): the handle carries a position, the inputs taken since the last period boundary
  // (0 .. down - 1, one number for all streams; 0 at creation and after reset()), and processAny(n) writes the outputs whose
  // newest input lies in the call -- outCountAny(n) of them from the current position, possibly none -- and moves it on.
  // inCountAny(nOut): the fewest inputs that write at least nOut.  position / setPosition: the by-hand carry beside state / setState.
  get position() { return addon.ratecvtPosition(this.handle); }
  setPosition(pos) {
    if (!(Number.isInteger(pos) && pos >= 0 && pos < this.down)) throw new RangeError('position ' + pos + ' outside 0..' + (this.down - 1));
    addon.ratecvtSetPosition(this.handle, pos);
  }
  outCountAny(nIn) { return addon.ratecvtOutCountAny(this.handle, nIn); }
  inCountAny(nOut) { return addon.ratecvtInCountAny(this.handle, nOut); }
  // an object of this class over a handle the library created (remap, restore)
  static adopt(handle, design) {
    const o = Object.create(this.prototype);
    o.inRate = design.inRate; o.outRate = design.outRate; o.up = design.up; o.down = design.down; o.taps = [...design.taps];
    o.handle = handle;
    o.nStreams = addon.ratecvtStreams(handle);
    o.history = addon.ratecvtHistory(handle);
    return o;
  }
  // fskhip_ratecvt_remap: a new object of this design, at this position, whose stream i continues stream map[i] of this one (its
  // history row, bit for bit; -1: a zero history) -- the map the engine and the processor were remapped with.  This object stays usable.
  remap(map) { return this.constructor.adopt(addon.ratecvtRemap(this.handle, Array.from(map)), this); }
  // fskhip_ratecvt_snapshot: the image of `streams` (null: all, in order) as a Buffer -- the design, the position and the history rows
  snapshot(streams = null) { return addon.ratecvtSnapshot(this.handle, streams === null || streams === undefined ? null : Array.from(streams)); }
  // fskhip_ratecvt_restore: a new object from a snapshot() alone, at the image's position; stream i continues record map[i] (-1: a
  // zero history; null: every record, in order).  `device`: the device's index, or { device, inRate, outRate } -- an image knows
  // up and down, not the rates: without them inRate / outRate are down / up, and rates of another ratio are refused.
  // CaptureConverter and PlaybackConverter refuse an image of the other direction; the class they share picks from the image.
  static fromSnapshot(buf, map = null, device = 0) {
    const options = typeof device === 'object' && device !== null ? device : { device };
    const info = addon.ratecvtSnapshotInfo(buf);
    if (this.DIRECTION !== undefined && info.direction !== this.DIRECTION) {
      throw new RangeError('the snapshot is of a rate converter for ' + ['capture', 'playback'][info.direction] + ', not ' + ['capture', 'playback'][this.DIRECTION]);
    }
    let inRate = info.down, outRate = info.up;
    if (options.inRate !== undefined || options.outRate !== undefined) {
      const r = RateConverter.ratio(options.inRate, options.outRate);
      if (r.up !== info.up || r.down !== info.down) {
        throw new RangeError(options.inRate + ' -> ' + options.outRate + ' is ' + r.up + ' / ' + r.down + ', the snapshot converts by ' + info.up + ' / ' + info.down);
      }
      inRate = options.inRate; outRate = options.outRate;
    }
    const handle = addon.ratecvtRestore(buf, map === null || map === undefined ? null : Array.from(map), options.device || 0);
    const kind = this.DIRECTION !== undefined ? this : [CaptureConverter, PlaybackConverter][info.direction];
    return kind.adopt(handle, { inRate, outRate, up: info.up, down: info.down, taps: Array.from(info.taps) });
  }
}
function ratecvtSnapshotInfo(buf) { return addon.ratecvtSnapshotInfo(buf); }
class CaptureConverter extends RateConverter {
  static get DIRECTION() { return 0; }
  constructor(inRate, outRate, nStreams, options = {}) { super(0, inRate, outRate, nStreams, options); }
  // samples: the format's typed array, [nStreams][pitch] (layout 'stream') or frames [nIn][pitch >= nStreams] ('sample'); nIn (a
  // multiple of down) and pitch default to a packed array's -> Float32Array [nStreams][nIn / down * up]
  process(samples, format, layout = 'stream', nIn, pitch) { return rateWiden(this, addon.ratecvtCapture, samples, format, layout, nIn, pitch, (n) => this.outCount(n)); }
  // process() for any nIn, from the handle's position -> Float32Array [nStreams][outCountAny(nIn)]
  processAny(samples, format, layout = 'stream', nIn, pitch) { return rateWiden(this, addon.ratecvtCaptureAny, samples, format, layout, nIn, pitch, (n) => this.outCountAny(n)); }
}
class PlaybackConverter extends RateConverter {
  static get DIRECTION() { return 1; }
  constructor(inRate, outRate, nStreams, options = {}) { super(1, inRate, outRate, nStreams, options); }
  // input: Float32Array [nStreams][n], n a multiple of down; lens (Uint32Array or null): stream s reads as 0.0 from lens[s] on
  // -> the format's typed array, [nStreams][n / down * up] or frames [n / down * up][nStreams]
  process(input, format, layout = 'stream', lens = null) { return rateNarrow(this, addon.ratecvtPlayback, input, format, layout, lens, (n) => this.outCount(n)); }
  // process() for any n, from the handle's position -> [nStreams][outCountAny(n)] or frames; lens count from the call's first input
  processAny(input, format, layout = 'stream', lens = null) { return rateNarrow(this, addon.ratecvtPlaybackAny, input, format, layout, lens, (n) => this.outCountAny(n)); }
  // output samples that can be non-zero for a signal of n input samples
  outLength(n) { return n ? Math.floor(((n - 1) * this.up + this.taps.length - 1) / this.down) + 1 : 0; }
}

class IIRFilterBatch {                            // filters.ts:8-106, S streams per call
  constructor(b, a, nStreams = 1, options = {}) {
    // the constructor's three errors (filters.ts:19-21), before anything touches the GPU
    if (!b || b.length === 0) throw new Error('Feedforward coefficients (b) cannot be empty');
    if (!a || a.length === 0) throw new Error('Feedback coefficients (a) cannot be empty');
    if (a[0] === 0) throw new Error('First feedback coefficient (a[0]) cannot be zero');
    this.nStreams = nStreams;
    this.handle = addon.iirCreate(Float64Array.from(b), Float64Array.from(a), nStreams, options.device || 0,
      options.precision === undefined ? PRECISION_F64 : options.precision);
  }
  // Float32Array [nStreams][n] -> Float32Array (processBuffer, filters.ts:81-87)
  processBuffer(input) {
    const n = samplesPerStream(input, this.nStreams);
    if (n === 0) return new Float32Array(0);
    return addon.iirProcess(this.handle, input, n, n, this.nStreams);
  }
  // Float64Array [nStreams][n] -> Float64Array: what process() returns sample by sample (nothing rounded to float)
  processSamples(input) {
    const n = samplesPerStream(input, this.nStreams);
    if (n === 0) return new Float64Array(0);
    return addon.iirProcess(this.handle, input, n, n, this.nStreams);
  }
  reset(stream = -1) { addon.iirReset(this.handle, stream); }
  getCoefficients() {
    const c = addon.iirCoefficients(this.handle), nb = c[0], na = c[1];
    return { b: Array.from(c.subarray(2, 2 + nb)), a: Array.from(c.subarray(2 + nb, 2 + nb + na)) };
  }
  close() { if (this.handle) { addon.iirDestroy(this.handle); this.handle = null; } }
}

class IIRFilter extends IIRFilterBatch {          // filters.ts:8-106
  constructor(b, a, options = {}) { super(b, a, 1, options); }
  process(input) { return this.processSamples(Float64Array.of(input))[0]; }
}

class FilterFactory {                             // filters.ts:325-368
  static createIIRLowpass(cutoffFreq, sampleRate) { const d = FilterDesign.butterworthLowpass(cutoffFreq, sampleRate); return new IIRFilter(d.b, d.a); }
  static createIIRHighpass(cutoffFreq, sampleRate) { const d = FilterDesign.butterworthHighpass(cutoffFreq, sampleRate); return new IIRFilter(d.b, d.a); }
  static createIIRBandpass(centerFreq, bandwidth, sampleRate) { const d = FilterDesign.butterworthBandpass(centerFreq, bandwidth, sampleRate); return new IIRFilter(d.b, d.a); }
  static createFIRLowpass(cutoffFreq, sampleRate, numTaps = 51) { return new FIRFilter(FilterDesign.sincLowpass(cutoffFreq, sampleRate, numTaps)); }
  static createFIRHighpass(cutoffFreq, sampleRate, numTaps = 51) { return new FIRFilter(FilterDesign.sincHighpass(cutoffFreq, sampleRate, numTaps)); }
  static createFIRBandpass(centerFreq, bandwidth, sampleRate, numTaps = 51) { return new FIRFilter(FilterDesign.sincBandpass(centerFreq, bandwidth, sampleRate, numTaps)); }
}
module.exports = { FilterDesign, IIRFilter, IIRFilterBatch, FIRFilter, FIRFilterBatch, Upsampler, Downsampler, CaptureConverter, PlaybackConverter, resamplerSnapshotInfo, ratecvtSnapshotInfo, FilterFactory, PRECISION_F32, PRECISION_F64 };
