'use strict';
// FSKProcessorBatch.remap / snapshot / fromSnapshot through the N-API addon on the GPU (include/fskhip_next.h): rings and a
// mid-signal modulation continue across the cut -- every stream of the remapped and of the restored batch equals stream map[i] of
// a control batch that was never remapped and was fed the same calls; new streams (-1) start empty.
// usage: node processor_remap_test.js gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));
const P = require(path.join(__dirname, '..', '..', 'napi', 'fsk-processor.js'));

const S = 70, Q = 128;

function signals(n) {
  const mod = new M.FSKBatch(S, {});
  const frames = mod.modulateData(Array.from({ length: S }, (_, s) => Uint8Array.from({ length: 12 + (s % 9) }, (_v, j) => (s * 31 + j * 7) & 0xff)));
  mod.close();
  const x = new Float32Array(S * n);
  for (let s = 0; s < S; s++) x.set(frames[s].subarray(0, n - (s % 13) * 64), s * n + (s % 13) * 64);
  return x;
}
function quantum(x, n, idx, q) {
  const out = new Float32Array(idx.length * Q);
  idx.forEach((r, i) => { if (r >= 0) out.set(x.subarray(r * n + q * Q, r * n + (q + 1) * Q), i * Q); });
  return out;
}
function rowsOf(a, i) { return Array.from(a.subarray(i * Q, (i + 1) * Q)); }

function gpuTests() {
  const quanta = 90, cut = 40, n = quanta * Q;
  const x = signals(n);
  const all = Array.from({ length: S }, (_, s) => s);
  const opts = { precision: M.PRECISION_F64 };
  const make = () => new P.FSKProcessorBatch(new M.FSKBatch(S, {}, opts), { rxCapacity: 48 });
  const ctrl = make(), src = make();
  const payloads = all.map((s) => Uint8Array.from({ length: s % 7 }, (_v, j) => (s + j) & 0xff));   // (some empty: pending for ever)
  const mask = all.map((s) => s % 3 !== 1);
  for (let q = 0; q < cut; q++) {
    if (q === cut - 6) for (const b of [ctrl, src]) b.modulate(payloads, mask);
    if (q === 25) for (const b of [ctrl, src]) b.demodulate();
    const a = ctrl.process(quantum(x, n, all, q), Q, Q), b = src.process(quantum(x, n, all, q), Q, Q);
    assert.deepStrictEqual(Array.from(a), Array.from(b));
  }
  const map = [];
  for (let i = 0; i < 55; i++) map.push(i % 9 === 4 ? -1 : (i * 29 + 3) % S);     // permutes, drops, duplicates; new slots
  const remapped = src.remap(map);
  const snap = src.snapshot();
  assert.ok(Buffer.isBuffer(snap.engine) && Buffer.isBuffer(snap.processor));
  assert.strictEqual(P.processorSnapshotInfo(snap.processor).nStreams, S);
  assert.strictEqual(P.processorSnapshotInfo(snap.processor).rxCapacity, 48);
  assert.deepStrictEqual(src.snapshot().processor, snap.processor);              // deterministic
  const restored = P.FSKProcessorBatch.fromSnapshot(snap, map);
  assert.strictEqual(remapped.processDemodulationCallCount, cut);
  assert.strictEqual(restored.processDemodulationCallCount, 0);
  assert.deepStrictEqual(remapped.snapshot().processor, restored.snapshot().processor);
  const tx0 = ctrl.txState();
  assert.ok(all.some((s) => tx0.pending[s] && tx0.pos[s] > 0), 'a modulation is mid-signal at the cut');
  assert.ok(Array.from(ctrl.rxLengths()).some((v) => v > 0), 'rings hold bytes at the cut');
  for (const b of [remapped, restored]) {
    const tx = b.txState(), len = b.rxLengths(), cl = ctrl.rxLengths();
    map.forEach((s, i) => {
      for (const k of ['pos', 'total', 'pending', 'completed']) assert.strictEqual(tx[k][i], s < 0 ? 0 : tx0[k][s], k + ' ' + i);
      assert.strictEqual(len[i], s < 0 ? 0 : cl[s], 'length ' + i);
    });
  }
  for (let q = cut; q < quanta; q++) {
    const c = ctrl.process(quantum(x, n, all, q), Q, Q);
    const drain = q === 60 || q === quanta - 1;
    const cd = drain ? ctrl.demodulate() : null;
    const ctx = ctrl.txState();
    for (const b of [remapped, restored]) {
      const o = b.process(quantum(x, n, map, q), Q, Q);
      const d = drain ? b.demodulate() : null;
      const tx = b.txState();
      map.forEach((s, i) => {
        if (s < 0) { assert.ok(rowsOf(o, i).every((v) => v === 0)); return; }
        assert.deepStrictEqual(rowsOf(o, i), rowsOf(c, s), 'output ' + q + ' ' + i);
        assert.strictEqual(tx.completed[i], ctx.completed[s], 'completed ' + i);
        if (drain) assert.deepStrictEqual(Array.from(d[i]), Array.from(cd[s]), 'drain ' + q + ' ' + i);
      });
    }
  }
  assert.ok(Array.from(ctrl.txState().completed).some((v) => v > 0));
  assert.throws(() => src.remap([S]), /source has 70 streams/);
  for (const b of [remapped, restored, ctrl, src]) { b.close(); b.batch.close(); }
  console.log('js processor remap gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'gpu') gpuTests();
