'use strict';
// FSKProcessorBatch.processSamplesAt through the N-API addon (include/fskhip_next.h, fskhip_processor_process_rate_host).
//   cpu  the argument checks of napi/fsk-processor.js and of the addon, which come before any device call
//   gpu  two shapes (mu-law frames, s16 rows): TX -- processSamplesAt equals Downsampler.process over process() on a twin with a twin
//        handle, element for element, across the quanta in which the modulations complete and ring out; RX -- a processor fed those
//        samples through processSamplesAt ends every quantum with the snapshot of a twin fed Upsampler.process through process(); the
//        handles' histories equal the twins' after every quantum
// usage: node processor_rate_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

function cpuTests() {
  const b = Object.create(P.FSKProcessorBatch.prototype);      // the checks need the stream count only
  Object.assign(b, { nStreams: 3, flags: 0, handle: null, processDemodulationCallCount: 0 });
  const fake = (kind, nStreams) => Object.assign(Object.create(kind.prototype), { nStreams, handle: null });
  const up = fake(F.Upsampler, 3), down = fake(F.Downsampler, 3);
  const frames = new Uint8Array(24);
  assert.throws(() => b.processSamplesAt(null, { format: 'pcm24' }), /unknown sample format pcm24/);
  assert.throws(() => b.processSamplesAt(null, {}, { format: 7, nOut: 8, downsampler: down }), /unknown sample format 7/);
  assert.throws(() => b.processSamplesAt(null, { layout: 'planar' }), /unknown layout planar/);
  assert.throws(() => b.processSamplesAt(null, {}, { layout: 2, nOut: 8, downsampler: down }), /unknown layout 2/);
  assert.throws(() => b.processSamplesAt(null, null), TypeError);
  assert.throws(() => b.processSamplesAt(null, {}, 5), TypeError);
  assert.throws(() => b.processSamplesAt([1, 2, 3], { nIn: 1, upsampler: up }), /typed array or null/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: -1, upsampler: up }), RangeError);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8.5, upsampler: up }), RangeError);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 2 ** 32, downsampler: down }), RangeError);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 8, pitch: -3, downsampler: down }), RangeError);
  // the handles: there, of the right class and of the batch's stream count -- for a side that has samples
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8 }), /upsampler must be an Upsampler/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8, upsampler: down }), /upsampler must be an Upsampler/);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 8 }), /downsampler must be an Downsampler/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8, upsampler: up }, { nOut: 8, downsampler: up }), /downsampler must be an Downsampler/);
  assert.throws(() => b.processSamplesAt(frames, { nIn: 8, upsampler: fake(F.Upsampler, 4) }), /upsampler has 4 streams, the batch 3/);
  assert.throws(() => b.processSamplesAt(null, {}, { nOut: 8, downsampler: fake(F.Downsampler, 2) }), /downsampler has 2 streams, the batch 3/);
  assert.strictEqual(b.processDemodulationCallCount, 0);
  // the addon's own: argument count, then format and layout (addon_util.h's TypeError), before the handle is looked at
  const A = M.addon;
  assert.strictEqual(typeof A.processorProcessSamplesAt, 'function');
  assert.throws(() => A.processorProcessSamplesAt(null, null, null, null, 0, 0), /too few arguments/);
  assert.throws(() => A.processorProcessSamplesAt(null, null, null, null, 9, 0, 0, 0, 0, 0, 0, 0, 0), (e) => e instanceof TypeError && /unknown sample format or layout/.test(e.message));
  assert.throws(() => A.processorProcessSamplesAt(null, null, null, null, 1, 0, 0, 0, 2, 3, 0, 0, 0), (e) => e instanceof TypeError && /unknown sample format or layout/.test(e.message));
  assert.throws(() => A.processorProcessSamplesAt(null, null, null, null, 1, 0, 0, 0, 2, 1, 0, 0, 0), /processor destroyed/);
  console.log('js processor rate cpu tests ok');
}

function gpuTests() {
  const S = 66, Q = 160, L = 6;    // one whole 64-stream group and a partial one; a 20 ms packet at 8 kHz; 8 kHz <-> 48 kHz
  const mk = () => { const batch = new M.FSKBatch(S, {}); return { batch, proc: new P.FSKProcessorBatch(batch, { rxCapacity: 16 }) }; };
  const same = (a, b, what) => {
    const x = a.proc.snapshot(), y = b.proc.snapshot();
    assert.ok(Buffer.compare(x.engine, y.engine) === 0 && Buffer.compare(x.processor, y.processor) === 0, what + ': snapshots differ');
  };
  const equal = (a, b, what) => {
    assert.strictEqual(a.length, b.length, what + ': length');
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i] && !(Number.isNaN(a[i]) && Number.isNaN(b[i]))) assert.fail(what + ': element ' + i + ': got ' + a[i] + ', want ' + b[i]);
  };
  const payload = (s) => Uint8Array.from({ length: s === 0 ? 0 : s === 1 ? 1 : 2 + s % 2 }, (_, i) => (s * 29 + 11 * i + 3) & 0xff);   // one empty, one a single byte
  for (const [fmt, lay, type] of [['mulaw', 'sample', Uint8Array], ['s16', 'stream', Int16Array]]) {
    const txRef = mk(), txDut = mk(), rxRef = mk(), rxDut = mk();
    const dnRef = new F.Downsampler(L, S), dnDut = new F.Downsampler(L, S), upRef = new F.Upsampler(L, S), upDut = new F.Upsampler(L, S);
    const payloads = Array.from({ length: S }, (_, s) => payload(s));
    txRef.proc.modulate(payloads);
    txDut.proc.modulate(payloads);
    const longest = Math.max(...txRef.proc.txState().total);
    for (let q = 0; q * Q * L < longest + 2 * Q * L; q++) {
      const what = fmt + ' ' + lay + ' quantum ' + q;
      const want = dnRef.process(txRef.proc.process(null, 0, Q * L), fmt, lay);
      const got = txDut.proc.processSamplesAt(null, {}, { format: fmt, layout: lay, nOut: Q, downsampler: dnDut });
      assert.ok(got instanceof type, what + ': type');
      equal(got, want, what + ' tx');
      equal(dnDut.state(), dnRef.state(), what + ' decimator history');
      same(txRef, txDut, what + ' tx');
      // RX: the samples as they came out; the twin takes the interpolated floats
      rxRef.proc.process(upRef.process(got, fmt, lay, Q), Q * L, 0);
      assert.strictEqual(rxDut.proc.processSamplesAt(got, { format: fmt, layout: lay, nIn: Q, upsampler: upDut }), null);
      equal(upDut.state(), upRef.state(), what + ' interpolator history');
      same(rxRef, rxDut, what + ' rx');
    }
    const tx = txDut.proc.txState();
    for (let s = 0; s < S; s++) assert.strictEqual(tx.pending[s], s === 0 ? 1 : 0, 'pending ' + s);
    const a = rxRef.proc.demodulate(), b = rxDut.proc.demodulate();
    for (let s = 0; s < S; s++) {
      assert.deepStrictEqual(Array.from(b[s]), Array.from(a[s]), 'bytes ' + s);
      assert.deepStrictEqual(Array.from(b[s]), Array.from(payloads[s]), 'payload ' + s);      // the link carries the bytes
    }
    assert.strictEqual(rxDut.proc.processDemodulationCallCount, rxRef.proc.processDemodulationCallCount);
    // the addon's own refusals on a live processor; the library's, with its message
    assert.throws(() => rxDut.proc.processSamplesAt(new type(8), { format: fmt, layout: lay, nIn: Q, upsampler: upDut }), /input too short/);
    assert.throws(() => rxDut.proc.processSamplesAt(null, {}, { format: fmt, layout: lay, nOut: Q, pitch: 2, downsampler: dnDut }), /output pitch too small/);
    assert.throws(() => M.addon.processorProcessSamplesAt(rxDut.proc.handle, dnDut.handle, null, new Uint8Array(S * Q), 2, 1, Q, S, 2, 1, 0, S, 0), /the up handle resamples down/);
    equal(upDut.state(), upRef.state(), 'a refused call leaves the history');
    for (const x of [dnRef, dnDut, upRef, upDut]) x.close();
    for (const x of [txRef, txDut, rxRef, rxDut]) { x.proc.close(); x.batch.close(); }
  }
  console.log('js processor rate gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'cpu') cpuTests(); else gpuTests();
