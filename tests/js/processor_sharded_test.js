'use strict';
// FSKProcessorBatchSharded (napi/fsk-processor.js) against its twin: one FSKProcessorBatch of the same 70 streams fed the same calls,
// bit for bit.  The shards are 35 + 35 on devices [0, 0] and 24 + 23 + 23 on [0, 0, 0].  The line is a loopback: a quantum's input
// is the output of the quantum before it, moved on by one stream.  usage: node processor_sharded_test.js cpu|gpu
const assert = require('assert');
const path = require('path');
const N = path.join(__dirname, '..', '..', 'napi');
const { FSKBatch } = require(path.join(N, 'fsk-core.js'));
const P = require(path.join(N, 'fsk-processor.js'));
const mode = process.argv[2] || 'cpu';
const S = 70;
const LENS = [128, 128, 128, 128, 1].concat(new Array(6).fill(128), [129], new Array(10).fill(128));   // 22 quanta, 2 690 samples
const SECOND_AT = 15;

function cpuTests() {
  assert.strictEqual(typeof P.FSKProcessorBatchSharded, 'function');
  assert.strictEqual(typeof P.processorSnapshotConcat, 'function');
  assert.deepStrictEqual(P.FSKProcessorBatchSharded.blocks(70, [0, 0]).map((b) => [b.first, b.count]), [[0, 35], [35, 35]]);
  assert.deepStrictEqual(P.FSKProcessorBatchSharded.blocks(70, [4, 5, 6]).map((b) => [b.first, b.count, b.device]), [[0, 24, 4], [24, 23, 5], [47, 23, 6]]);
  assert.deepStrictEqual(P.FSKProcessorBatchSharded.blocks(2, [0, 1, 2]).map((b) => b.count), [1, 1]);
  for (const m of ['process', 'processSamples', 'processSamplesAt', 'processSamplesAtAny', 'modulate', 'rxDrainSparse', 'remap', 'snapshot', 'close']) {
    assert.strictEqual(typeof P.FSKProcessorBatchSharded.prototype[m], 'function', m);
  }
  assert.strictEqual(typeof P.FSKProcessorBatchSharded.fromSnapshot, 'function');
  assert.throws(() => P.processorSnapshotConcat([]));
  console.log('js processor sharded cpu tests ok');
}

const payloads = (seed, keep) => Array.from({ length: S }, (_, s) => (keep(s) ? Uint8Array.from({ length: 1 + ((Math.floor(s / 3) + seed) % 3) }, (_, i) => (s * 7 + i * 13 + seed) & 0xff) : new Uint8Array(0)));
const same = (a, b, what) => assert.ok(Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)), what);

function assertSame(ref, dut, where) {
  same(ref.rxLengths(), dut.rxLengths(), where + ' rxLengths');
  const a = ref.txState(), b = dut.txState();
  for (const k of ['pos', 'total', 'pending', 'completed']) same(a[k], b[k], where + ' txState.' + k);
  for (let s = 0; s < S; s++) assert.deepStrictEqual(dut.status(s), ref.status(s), where + ' status ' + s);
}

// one quantum on every batch (batches[0] is the twin); frames of a sharded batch go into one caller-owned out between two guard columns
function quantum(batches, fmt, x, nIn, nOut, q) {
  const outs = batches.map((b) => {
    if (fmt === 'f32') return q % 2 ? b.processSamples(x, { nIn }, { nOut }) : b.process(x, nIn, nOut);
    if (!(b instanceof P.FSKProcessorBatchSharded)) return b.processSamples(x, { format: fmt, layout: 'sample', nIn }, { format: fmt, layout: 'sample', nOut });
    const Arr = fmt === 's16' ? Int16Array : Uint8Array, pitch = S + 2;
    const guard = new Arr(pitch * nOut + 1).fill(0x5a);
    const got = b.processSamples(x, { format: fmt, layout: 'sample', nIn }, { format: fmt, layout: 'sample', nOut, pitch, out: guard.subarray(1) });
    assert.strictEqual(got.buffer, guard.buffer);
    const packed = new Arr(nOut * S);
    for (let i = 0; i < nOut; i++) {
      assert.ok(guard[i * pitch] === 0x5a && guard[i * pitch + S + 1] === 0x5a, 'guard columns, quantum ' + q);
      packed.set(guard.subarray(1 + i * pitch, 1 + i * pitch + S), i * S);
    }
    return packed;
  });
  outs.slice(1).forEach((o, k) => { same(o, outs[0], 'output, quantum ' + q + ' batch ' + (k + 1)); assertSame(batches[0], batches[k + 1], 'quantum ' + q + ' batch ' + (k + 1)); });
  return outs[0];
}

function roll(out, fmt, n) {            // the next input: every stream hears the one before it
  const x = new out.constructor(out.length);
  if (fmt === 'f32') for (let s = 0; s < S; s++) x.set(out.subarray(s * n, (s + 1) * n), ((s + 1) % S) * n);
  else for (let i = 0; i < n; i++) for (let s = 0; s < S; s++) x[i * S + ((s + 1) % S)] = out[i * S + s];
  return x;
}

function drive(batches, fmt, lens, x0, q0) {
  const Arr = fmt === 'f32' ? Float32Array : fmt === 's16' ? Int16Array : Uint8Array;
  let x = x0 || new Arr(lens[0] * S).fill(fmt === 'mulaw' ? 0xff : 0), nIn = x.length / S;
  lens.forEach((n, i) => {
    const q = q0 + i;
    if (q === 0) batches.forEach((b) => b.modulate(payloads(1, (s) => s % 3 === 0), Array.from({ length: S }, (_, s) => s % 3 === 0)));
    if (q === SECOND_AT) batches.forEach((b) => b.modulate(payloads(2, (s) => s % 3 === 1), Array.from({ length: S }, (_, s) => s % 3 === 1)));
    x = roll(quantum(batches, fmt, x, nIn, n, q), fmt, n);
    nIn = n;
  });
  return x;
}

const pair = (devices, precision) => [new P.FSKProcessorBatch(new FSKBatch(S, {}, { device: 0, precision }), { clearRxOnTxComplete: false }),
  new P.FSKProcessorBatchSharded(S, {}, { devices, precision, clearRxOnTxComplete: false })];
const closeAll = (bs) => bs.forEach((b) => { const batch = b.batch; b.close(); if (batch) batch.close(); });

function midFrame(twin) {
  const t = twin.txState();
  let sending = 0, holding = 0;
  const lens = twin.rxLengths();
  for (let s = 0; s < S; s++) { if (t.pending[s] && t.pos[s] > 0 && t.pos[s] < t.total[s]) sending++; if (lens[s]) holding++; }
  assert.ok(sending >= 10 && holding >= 10, 'mid-frame: ' + sending + ' sending, ' + holding + ' holding bytes');
}

function gpuTests() {
  // 1. quantum parity
  for (const [fmt, devices, precision] of [['f32', [0, 0], 0], ['s16', [0, 0, 0], 0], ['mulaw', [0, 0], 0], ['f32', [0, 0, 0], 1], ['s16', [0, 0], 1]]) {
    const bs = pair(devices, precision);
    try {
      assert.deepStrictEqual(bs[1].shards.map((sh) => sh.count), devices.length === 2 ? [35, 35] : [24, 23, 23]);
      drive(bs, fmt, LENS, null, 0);
      midFrame(bs[0]);
      assert.strictEqual(bs[1].processDemodulationCallCount, LENS.length);
      assert.deepStrictEqual(bs[1].lastTxKernel, devices.map(() => bs[0].lastTxKernel));
      const mask = Array.from({ length: S }, (_, s) => s % 5 !== 2);
      const a = bs[0].rxDrainSparse({ mask, minLen: 3 }), b = bs[1].rxDrainSparse({ mask, minLen: 3 });
      assert.ok(a.streams.length >= 3);
      same(a.streams, b.streams, 'sparse streams'); same(a.offsets, b.offsets, 'sparse offsets'); same(a.data.subarray(0, a.offsets[a.streams.length]), b.data, 'sparse data');
      const da = bs[0].demodulate(), db = bs[1].demodulate();
      da.forEach((r, s) => same(r, db[s], 'demodulate ' + s));
    } finally { closeAll(bs); }
  }
  // 2. images, 3. rebalancing
  for (const precision of [0, 1]) {
    const bs = pair([0, 0], precision);
    const made = [];
    try {
      const x = drive(bs, 's16', LENS, null, 0);
      midFrame(bs[0]);
      const a = bs[0].snapshot(), b = bs[1].snapshot();
      assert.ok(Buffer.from(b.processor).equals(Buffer.from(a.processor)), 'the sharded processor image is the twin\'s, byte for byte');
      const single = P.FSKProcessorBatch.fromSnapshot(b, undefined, undefined, 0, { clearRxOnTxComplete: false });
      const sharded = P.FSKProcessorBatchSharded.fromSnapshot(a, undefined, undefined, { devices: [0, 0, 0], clearRxOnTxComplete: false });
      made.push(single, sharded);
      assert.strictEqual(single.processDemodulationCallCount, 0);
      assert.strictEqual(sharded.processDemodulationCallCount, 0);
      single.processDemodulationCallCount = sharded.processDemodulationCallCount = LENS.length;    // (status() reports the host counter)
      for (const dut of [single, sharded]) { assertSame(bs[0], dut, 'restored'); assert.ok(Buffer.from(dut.snapshot().processor).equals(Buffer.from(a.processor))); }
      // a permutation with 13 sources named twice and 5 new streams, taken mid-frame
      const src = Array.from({ length: S }, (_, i) => (i * 37 + 11) % S);
      const m = src.slice(0, S - 18).concat(src.slice(3, 16), [-1, -1, -1, -1, -1]);
      for (let i = m.length - 1; i > 0; i--) { const j = (i * 29 + 7) % (i + 1); const t = m[i]; m[i] = m[j]; m[j] = t; }
      assert.strictEqual(m.length, S);
      const moved = [bs[0].remap(m), bs[1].remap(m, undefined, { devices: [0, 0, 0] }), bs[1].remap(m, undefined, { devices: [0] })];
      made.push(...moved);
      assert.deepStrictEqual(moved.map((v) => v.processDemodulationCallCount), [LENS.length, LENS.length, LENS.length]);
      assert.deepStrictEqual(moved[1].shards.map((sh) => sh.count), [24, 23, 23]);
      assertSame(moved[0], moved[1], 'remapped to three shards'); assertSame(moved[0], moved[2], 'remapped to one shard');
      drive([bs[0], bs[1], single, sharded], 's16', [128, 129, 128], x, LENS.length);
      const x2 = new Int16Array(x.length), n = x.length / S;
      for (let i = 0; i < n; i++) for (let s = 0; s < S; s++) x2[i * S + s] = m[s] >= 0 ? x[i * S + m[s]] : 0;
      drive(moved, 's16', [128, 1, 129], x2, LENS.length);
    } finally { closeAll(bs.concat(made)); }
  }
  console.log('js processor sharded gpu tests ok');
}

if (mode === 'gpu') gpuTests(); else cpuTests();
