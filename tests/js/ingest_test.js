'use strict';
// FSKBatch.demodulateSamples through the N-API addon on the GPU (include/fskhip.h, fskhip_demodulate_host_fmt): an Int16Array and a
// G.711 mu-law Uint8Array, stream-major and as interleaved frames, give what demodulateData gives on the floats this script
// converts itself -- bytes, 'eod' counts, status -- on FSKBatch, its async form and FSKBatchSharded.  usage: node ingest_test.js gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));

const S = 66;   // one whole 64-stream group and a partial one

function mulawToLinear(b) {   // include/fskhip.h's formula
  const u = ~b & 0xff;
  const mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
  return (u & 0x80) ? -mag : mag;
}
const MULAW = Array.from({ length: 256 }, (_, b) => ({ b, v: mulawToLinear(b) / 32768 })).sort((p, q) => p.v - q.v);
function toMulaw(x) {         // the nearest entry of the decode table
  let lo = 0, hi = 255;
  while (hi - lo > 1) { const mid = (lo + hi) >> 1; if (MULAW[mid].v <= x) lo = mid; else hi = mid; }
  return (Math.abs(x - MULAW[lo].v) <= Math.abs(MULAW[hi].v - x) ? MULAW[lo] : MULAW[hi]).b;
}

function payload(s) { return Uint8Array.from({ length: 16 }, (_, i) => 0x41 + (s * 5 + 3 * i) % 26); }   // letters: every such frame decodes

function signal() {   // [S][n]: a staggered lead-in, one 16-byte frame at amplitude 0.5, silence
  const mod = new M.FSKBatch(S, {});
  const frames = mod.modulateData(Array.from({ length: S }, (_, s) => payload(s)));
  mod.close();
  const n = 399 + frames[0].length + 3000;
  const x = new Float32Array(S * n);
  for (let s = 0; s < S; s++) frames[s].forEach((v, i) => { x[s * n + (s * 7 % 400) + i] = 0.5 * v; });
  return { x, n };
}

function transposed(a, n, pitch) {   // [S][n] -> frames [n][pitch >= S]
  const t = new a.constructor(n * pitch);
  for (let s = 0; s < S; s++) for (let i = 0; i < n; i++) t[i * pitch + s] = a[s * n + i];
  return t;
}

function same(got, want, batch, ref, what) {
  for (let s = 0; s < S; s++) {
    assert.deepStrictEqual(Array.from(got.bytes[s]), Array.from(want.bytes[s]), what + ': bytes ' + s);
    assert.strictEqual(got.eod[s], want.eod[s], what + ': eod ' + s);
    if (batch) assert.deepStrictEqual(batch.getStatus(s), ref.getStatus(s), what + ': status ' + s);
  }
}

async function gpuTests() {
  const { x, n } = signal();
  const s16 = Int16Array.from(x, (v) => Math.max(-32768, Math.min(32767, Math.round(v * 32768))));
  const mu = Uint8Array.from(x, toMulaw);
  const cases = [
    ['s16', s16, Float32Array.from(s16, (v) => v / 32768)],
    ['mulaw', mu, Float32Array.from(mu, (b) => mulawToLinear(b) / 32768)],
  ];
  for (const [fmt, narrow, floats] of cases) {
    const ref = new M.FSKBatch(S, {});
    const want = ref.demodulateData(floats, n);
    for (let s = 0; s < S; s++) assert.deepStrictEqual(Array.from(want.bytes[s]), Array.from(payload(s)), fmt + ': the frame decodes ' + s);
    const frames = transposed(narrow, n, S + 3);
    for (const [layout, arr, pitch] of [['stream', narrow, n], ['sample', frames, S + 3]]) {
      const b = new M.FSKBatch(S, {});
      same(b.demodulateSamples(arr, fmt, layout, n, pitch), want, b, ref, fmt + ' ' + layout);
      b.close();
      const c = new M.FSKBatch(S, {});
      same(await c.demodulateSamplesAsync(arr, fmt, layout, n, pitch), want, c, ref, fmt + ' ' + layout + ' async');
      c.close();
      const sh = new M.FSKBatchSharded(S, {}, { devices: [0, 0] });   // two shards on one device: a row block / a column block each
      same(await sh.demodulateSamples(arr, fmt, layout, n, pitch), want, sh, ref, fmt + ' ' + layout + ' sharded');
      sh.close();
    }
    ref.close();
  }
  const b = new M.FSKBatch(S, {});
  assert.throws(() => b.demodulateSamples(s16, 'mulaw', 'stream', n), /typed array/);
  assert.throws(() => b.demodulateSamples(s16, 'pcm24', 'stream', n), /unknown sample format/);
  assert.throws(() => b.demodulateSamples(s16, 's16', 'planar', n), /unknown layout/);
  assert.throws(() => b.demodulateSamples(s16.subarray(1), 's16', 'stream', n), /samples too short/);
  assert.throws(() => b.demodulateSamples(s16, 's16', 'sample', n, S - 1), /samples too short/);
  b.close();
  console.log('js ingest gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'gpu') gpuTests().catch((e) => { console.error(e); process.exit(1); });
