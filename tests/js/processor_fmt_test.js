'use strict';
// FSKProcessorBatch.processSamples through the N-API addon (include/fskhip_next.h, fskhip_processor_process_fmt_host).
//   cpu  the argument checks of napi/fsk-processor.js and of the addon, which come before any device call
//   gpu  one shape: TX -- processSamples equals this script's encoding of process() on a twin, element for element, across the quantum
//        in which the modulations complete, sentinel columns of wider rows and frames untouched; RX -- a processor fed those samples
//        through processSamples ends every quantum with the snapshot of a twin fed the decoded floats through process()
// usage: node processor_fmt_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));

function toS16(x) {           // clamp(rne(x * 32768)), include/fskhip.h
  const y = Math.fround(x * 32768);
  if (Number.isNaN(y)) return 0;
  let r = Math.floor(y);
  const d = y - r;
  if (d > 0.5 || (d === 0.5 && (r & 1))) r += 1;
  return Math.max(-32768, Math.min(32767, r));
}
function toMulaw(v) {
  let m = v >> 2;
  const neg = m < 0;
  m = Math.min(Math.abs(m), 8158) + 33;
  const seg = 31 - Math.clz32(m) - 5;
  return ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ (neg ? 0x7f : 0xff);
}
function fromMulaw(b) {
  const u = ~b & 0xff;
  const mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
  return Math.fround(((u & 0x80) ? -mag : mag) / 32768);
}
const FORMATS = {
  s16: { type: Int16Array, enc: toS16, dec: (v) => Math.fround(v / 32768) },
  mulaw: { type: Uint8Array, enc: (x) => toMulaw(toS16(x)), dec: fromMulaw },
};

function cpuTests() {
  const b = Object.create(P.FSKProcessorBatch.prototype);      // the checks need the stream count only
  Object.assign(b, { nStreams: 3, flags: 0, handle: null, processDemodulationCallCount: 0 });
  assert.throws(() => b.processSamples(null, { format: 'pcm24' }), /unknown sample format pcm24/);
  assert.throws(() => b.processSamples(null, {}, { format: 7, nOut: 8 }), /unknown sample format 7/);
  assert.throws(() => b.processSamples(null, { layout: 'planar' }), /unknown layout planar/);
  assert.throws(() => b.processSamples(null, {}, { layout: 2, nOut: 8 }), /unknown layout 2/);
  assert.throws(() => b.processSamples(null, null), TypeError);
  assert.throws(() => b.processSamples(null, {}, 5), TypeError);
  assert.throws(() => b.processSamples([1, 2, 3], { format: 's16', nIn: 1 }), /typed array or null/);
  assert.throws(() => b.processSamples(new Int16Array(24), { format: 's16', nIn: -1 }), RangeError);
  assert.throws(() => b.processSamples(new Int16Array(24), { format: 's16', nIn: 8.5 }), RangeError);
  assert.throws(() => b.processSamples(null, {}, { nOut: 2 ** 32 }), RangeError);
  assert.throws(() => b.processSamples(null, {}, { nOut: 8, pitch: -3 }), RangeError);
  // the addon's own: argument count, then format and layout (addon_util.h's TypeError), before the handle is looked at
  const A = M.addon;
  assert.strictEqual(typeof A.processorProcessSamples, 'function');
  assert.throws(() => A.processorProcessSamples(null, null, 0, 0), /too few arguments/);
  assert.throws(() => A.processorProcessSamples(null, null, 9, 0, 0, 0, 0, 0, 0, 0, 0), (e) => e instanceof TypeError && /unknown sample format or layout/.test(e.message));
  assert.throws(() => A.processorProcessSamples(null, null, 1, 0, 0, 0, 2, 3, 0, 0, 0), (e) => e instanceof TypeError && /unknown sample format or layout/.test(e.message));
  assert.throws(() => A.processorProcessSamples(null, null, 1, 0, 0, 0, 2, 1, 0, 0, 0), /processor destroyed/);
  assert.strictEqual(b.processDemodulationCallCount, 0);
  console.log('js processor fmt cpu tests ok');
}

function gpuTests() {
  const S = 66, Q = 160;    // one whole 64-stream group and a partial one; a 20 ms RTP frame at 8 kHz
  const mk = () => { const batch = new M.FSKBatch(S, {}); return { batch, proc: new P.FSKProcessorBatch(batch, { rxCapacity: 16 }) }; };
  const same = (a, b, what) => {
    const x = a.proc.snapshot(), y = b.proc.snapshot();
    assert.ok(Buffer.compare(x.engine, y.engine) === 0 && Buffer.compare(x.processor, y.processor) === 0, what + ': snapshots differ');
  };
  const payload = (s) => Uint8Array.from({ length: s === 0 ? 0 : s === 1 ? 1 : 2 + s % 2 }, (_, i) => (s * 29 + 11 * i + 3) & 0xff);   // one empty, one a single byte
  for (const [fmt, lay] of [['mulaw', 'sample'], ['s16', 'stream']]) {
    const F = FORMATS[fmt];
    const txRef = mk(), txDut = mk(), rxRef = mk(), rxDut = mk();
    const payloads = Array.from({ length: S }, (_, s) => payload(s));
    txRef.proc.modulate(payloads);
    txDut.proc.modulate(payloads);
    const longest = Math.max(...txRef.proc.txState().total);
    const pitch = (lay === 'sample' ? S : Q) + 3;
    const at = (s, t) => (lay === 'sample' ? t * pitch + s : s * pitch + t);
    for (let q = 0; q * Q < longest + 2 * Q; q++) {
      const floats = txRef.proc.process(null, 0, Q);
      const got = txDut.proc.processSamples(null, {}, { format: fmt, layout: lay, nOut: Q, pitch });
      assert.ok(got instanceof F.type, fmt + ' ' + lay + ': type');
      for (let s = 0; s < S; s++) {
        for (let t = 0; t < Q; t++) {
          const want = F.enc(floats[s * Q + t]);
          const g = got[at(s, t)];
          if (g !== want) assert.fail(fmt + ' ' + lay + ' quantum ' + q + ': stream ' + s + ' sample ' + t + ': got ' + g + ', want ' + want);
        }
      }
      same(txRef, txDut, fmt + ' ' + lay + ' tx quantum ' + q);
      // RX: the samples as they came out, other values in the columns the batch does not own; the twin takes the decoded floats
      const wide = F.type.from(got);
      const rows = lay === 'sample' ? Q : S, cols = lay === 'sample' ? S : Q;
      for (let i = 0; i < rows - 1; i++) for (let j = cols; j < pitch; j++) wide[i * pitch + j] = 99;
      const dec = new Float32Array(S * Q);
      for (let s = 0; s < S; s++) for (let t = 0; t < Q; t++) dec[s * Q + t] = F.dec(got[at(s, t)]);
      rxRef.proc.process(dec, Q, 0);
      assert.strictEqual(rxDut.proc.processSamples(wide, { format: fmt, layout: lay, nIn: Q, pitch }), null);
      same(rxRef, rxDut, fmt + ' ' + lay + ' rx quantum ' + q);
    }
    const tx = txDut.proc.txState();
    for (let s = 0; s < S; s++) assert.strictEqual(tx.pending[s], s === 0 ? 1 : 0, 'pending ' + s);
    const a = rxRef.proc.demodulate(), b = rxDut.proc.demodulate();
    let heard = 0;
    for (let s = 0; s < S; s++) { assert.deepStrictEqual(Array.from(b[s]), Array.from(a[s]), 'bytes ' + s); heard += a[s].length; }
    assert.ok(heard > 0, 'no frame was heard');
    assert.strictEqual(rxDut.proc.processDemodulationCallCount, rxRef.proc.processDemodulationCallCount);
    assert.throws(() => rxDut.proc.processSamples(new F.type(8), { format: fmt, layout: lay, nIn: Q }), /input too short/);
    assert.throws(() => rxDut.proc.processSamples(null, {}, { format: fmt, layout: lay, nOut: Q, pitch: 2 }), /output pitch too small/);
    assert.throws(() => rxDut.proc.processSamples(new Float32Array(S * Q), { format: fmt, layout: lay, nIn: Q }), /typed array/);
    for (const x of [txRef, txDut, rxRef, rxDut]) { x.proc.close(); x.batch.close(); }
  }
  console.log('js processor fmt gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'cpu') cpuTests(); else gpuTests();
