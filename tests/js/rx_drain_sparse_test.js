'use strict';
// FSKProcessorBatch.rxDrainSparse through the N-API addon (include/fskhip_next.h: fskhip_processor_rx_drain_sparse_host).
// cpu: the argument checks, which are made before the library is called, and the addon's own refusal of a handle that is none.
// gpu: a batch whose rings hold different amounts -- some none -- is cloned (remap with the identity); rxDrainSparse on one clone
// lists exactly the streams for which demodulate() on the other returns bytes, with the same bytes, in CSR form; a mask and a
// minLen leave the other streams' bytes for a later call.
// usage: node rx_drain_sparse_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));
const addon = require(path.join(__dirname, '..', '..', 'napi', 'fsk_addon.node'));

function cpuTests() {
  assert.strictEqual(typeof P.FSKProcessorBatch.prototype.rxDrainSparse, 'function');
  assert.strictEqual(typeof addon.processorDrainSparse, 'function');
  const b = Object.create(P.FSKProcessorBatch.prototype);   // no device here: the checks come before the handle is used
  b.nStreams = 4; b.handle = null;
  assert.throws(() => b.rxDrainSparse(null), /options must be an object/);
  assert.throws(() => b.rxDrainSparse(7), /options must be an object/);
  for (const minLen of [-1, 1.5, '3', NaN, 2 ** 32]) assert.throws(() => b.rxDrainSparse({ minLen }), /minLen must be an integer/);
  assert.throws(() => b.rxDrainSparse({ mask: 5 }), /mask must be an array/);
  assert.throws(() => b.rxDrainSparse({ mask: [true, false] }), /one entry per stream \(4\)/);
  assert.throws(() => b.rxDrainSparse({ mask: new Uint8Array(5) }), /one entry per stream \(4\)/);
  // past the checks the call reaches the addon, which refuses what is no processor handle
  assert.throws(() => b.rxDrainSparse(), /processor destroyed/);
  assert.throws(() => b.rxDrainSparse({ mask: [1, 0, 0, 1], minLen: 0 }), /processor destroyed/);
  assert.throws(() => addon.processorDrainSparse(), /too few arguments/);
  console.log('js rx drain sparse cpu tests ok');
}

function gpuTests() {
  const S = 70, Q = 128, quanta = 60;
  const mod = new M.FSKBatch(S, {});
  // streams 0, 5, 10, ... stay silent: their rings stay empty
  const frames = mod.modulateData(Array.from({ length: S }, (_, s) => Uint8Array.from({ length: 3 + (s % 6) }, (_v, j) => (s * 17 + j * 5 + 1) & 0xff)));
  mod.close();
  const n = quanta * Q;
  const x = new Float32Array(S * n);
  for (let s = 0; s < S; s++) if (s % 5 !== 0) x.set(frames[s].subarray(0, n - (s % 4) * 64), s * n + (s % 4) * 64);
  const src = new P.FSKProcessorBatch(new M.FSKBatch(S, {}), { rxCapacity: 48 });
  for (let q = 0; q < quanta; q++) {
    const inp = new Float32Array(S * Q);
    for (let s = 0; s < S; s++) inp.set(x.subarray(s * n + q * Q, s * n + (q + 1) * Q), s * Q);
    src.process(inp, Q, 0);
  }
  const all = Array.from({ length: S }, (_, s) => s);
  const sparse = src.remap(all), dense = src.remap(all), masked = src.remap(all);
  const want = dense.demodulate();
  const holders = all.filter((s) => want[s].length > 0);
  assert.ok(holders.length > 20 && holders.length < S, 'some rings hold bytes, some do not');

  const r = sparse.rxDrainSparse();
  assert.ok(r.streams instanceof Uint32Array && r.offsets instanceof Uint32Array && r.data instanceof Uint8Array);
  assert.deepStrictEqual(Array.from(r.streams), holders);
  assert.strictEqual(r.offsets.length, holders.length + 1);
  assert.strictEqual(r.offsets[0], 0);
  assert.strictEqual(r.offsets[holders.length], r.data.length);
  holders.forEach((s, i) => assert.deepStrictEqual(Array.from(r.data.subarray(r.offsets[i], r.offsets[i + 1])), Array.from(want[s]), 'stream ' + s));
  assert.deepStrictEqual(sparse.snapshot().processor, dense.snapshot().processor);
  const none = sparse.rxDrainSparse();
  assert.deepStrictEqual([none.streams.length, Array.from(none.offsets), none.data.length], [0, [0], 0]);

  // a mask and a minLen: what either excludes stays for a later call
  const mask = all.map((s) => s % 2 === 0);
  const first = masked.rxDrainSparse({ mask, minLen: 5 });
  assert.deepStrictEqual(Array.from(first.streams), holders.filter((s) => mask[s] && want[s].length >= 5));
  const rest = masked.rxDrainSparse({ minLen: 0 });
  assert.deepStrictEqual(Array.from(rest.streams), holders.filter((s) => !(mask[s] && want[s].length >= 5)));
  for (const part of [first, rest])
    part.streams.forEach((s, i) => assert.deepStrictEqual(Array.from(part.data.subarray(part.offsets[i], part.offsets[i + 1])), Array.from(want[s])));
  assert.deepStrictEqual(masked.snapshot().processor, dense.snapshot().processor);
  assert.throws(() => addon.processorRemap(sparse.handle, src.handle, all), /used already/);   // a drained processor is a used one
  for (const b of [sparse, dense, masked, src]) { b.close(); b.batch.close(); }
  console.log('js rx drain sparse gpu tests ok');
}

if ((process.argv[2] || 'cpu') === 'gpu') gpuTests(); else cpuTests();
