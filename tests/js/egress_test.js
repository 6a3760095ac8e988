'use strict';
// FSKBatch.modulateSamples through the N-API addon on the GPU (include/fskhip.h, fskhip_modulate_host_fmt): every format, stream-major
// and as interleaved frames, against modulateData plus this script's own restatement of the header's encoders -- element for element,
// silence from lens[s] on --, on FSKBatch and on FSKBatchSharded; then the round trip through demodulateSamples.
// usage: node egress_test.js gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));

const S = 66;   // one whole 64-stream group and a partial one

function toS16(x) {           // clamp(rne(x * 32768)): Math.fround keeps the product a float (it is exact); ties to even by hand
  const y = Math.fround(x * 32768);
  if (Number.isNaN(y)) return 0;
  let r = Math.floor(y);
  const d = y - r;
  if (d > 0.5 || (d === 0.5 && (r & 1))) r += 1;
  return Math.max(-32768, Math.min(32767, r));
}
function toMulaw(v) {         // include/fskhip.h's formula
  let m = v >> 2;
  const neg = m < 0;
  m = Math.min(Math.abs(m), 8158) + 33;
  const seg = 31 - Math.clz32(m) - 5;
  return ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ (neg ? 0x7f : 0xff);
}
function toAlaw(v) {
  let m = v >> 3;
  const neg = m < 0;
  m = neg ? -m - 1 : m;
  const seg = Math.max(31 - Math.clz32(Math.max(m, 1)) - 4, 0);
  return ((seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 15)) ^ (neg ? 0x55 : 0xd5);
}
const FORMATS = {
  f32: { type: Float32Array, enc: (x) => x, silence: 0 },
  s16: { type: Int16Array, enc: toS16, silence: 0 },
  mulaw: { type: Uint8Array, enc: (x) => toMulaw(toS16(x)), silence: 0xff },
  alaw: { type: Uint8Array, enc: (x) => toAlaw(toS16(x)), silence: 0xd5 },
};

function ragged(s) { return Uint8Array.from({ length: (s * 7) % 12 }, (_, i) => (s * 31 + 7 * i + 1) & 0xff); }   // the first one empty
function letters(s) { return Uint8Array.from({ length: 16 }, (_, i) => 0x41 + (s * 5 + 3 * i) % 26); }            // every such frame decodes

function check(r, floats, fmt, lay, n, pitch, what) {
  const F = FORMATS[fmt];
  assert.ok(r.samples instanceof F.type, what + ': type');
  for (let s = 0; s < S; s++) {
    assert.strictEqual(r.lens[s], floats[s].length, what + ': lens ' + s);
    for (let t = 0; t < n; t++) {
      const want = t < r.lens[s] ? F.enc(floats[s][t]) : F.silence;
      const got = r.samples[lay === 'sample' ? t * pitch + s : s * pitch + t];
      if (got !== want) assert.fail(what + ': stream ' + s + ' sample ' + t + ': got ' + got + ', want ' + want);
    }
  }
}

async function gpuTests() {
  // the encoders themselves, at their edges
  assert.deepStrictEqual([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1, -1, Infinity, -Infinity, NaN, -0].map(toS16).map((v) => v + 0),
                         [0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 0, 0]);
  assert.deepStrictEqual([0, -1, 32767, -32768, 1000, -1000].map(toMulaw), [0xff, 0x7e, 0x80, 0x00, 0xce, 0x4e]);
  assert.deepStrictEqual([0, -1, 32767, -32768, 1000, -1000].map(toAlaw), [0xd5, 0x55, 0xaa, 0x2a, 0xfa, 0x7a]);

  const payloads = Array.from({ length: S }, (_, s) => ragged(s));
  const b = new M.FSKBatch(S, {});
  const floats = b.modulateData(payloads);
  const longest = Math.max(...floats.map((f) => f.length));
  const sh = new M.FSKBatchSharded(S, {}, { devices: [0, 0] });   // two shards on one device: a row block / a column block each
  for (const fmt of Object.keys(FORMATS)) {
    for (const lay of ['stream', 'sample']) {
      const r = b.modulateSamples(payloads, fmt, lay);
      assert.strictEqual(r.nPerStream, longest);
      assert.strictEqual(r.pitch, lay === 'sample' ? S : longest);
      check(r, floats, fmt, lay, r.nPerStream, r.pitch, fmt + ' ' + lay);
      // a longer call at a wider pitch into the caller's array: silence behind every signal, the other columns untouched
      const n = longest + 9, pitch = (lay === 'sample' ? S : n) + 3;
      const out = new FORMATS[fmt].type(pitch * (lay === 'sample' ? n : S)).fill(77);
      const w = b.modulateSamples(payloads, fmt, lay, n, pitch, out);
      assert.strictEqual(w.samples, out);
      check(w, floats, fmt, lay, n, pitch, fmt + ' ' + lay + ' wide');
      const rows = lay === 'sample' ? n : S, cols = lay === 'sample' ? S : n;
      for (let i = 0; i < rows; i++) for (let j = cols; j < pitch; j++) assert.strictEqual(out[i * pitch + j], 77, fmt + ' ' + lay + ': padding');
      const out2 = new FORMATS[fmt].type(out.length).fill(77);
      const v = sh.modulateSamples(payloads, fmt, lay, n, pitch, out2);
      assert.deepStrictEqual(Array.from(v.lens), Array.from(w.lens));
      assert.deepStrictEqual(out2, out, fmt + ' ' + lay + ' sharded');
      check(sh.modulateSamples(payloads, fmt, lay), floats, fmt, lay, longest, lay === 'sample' ? S : longest, fmt + ' ' + lay + ' sharded, own array');
    }
  }
  const s16 = new Int16Array(S * longest);
  assert.throws(() => b.modulateSamples(payloads, 'mulaw', 'stream', longest, longest, s16), /typed array/);
  assert.throws(() => b.modulateSamples(payloads, 'pcm24', 'stream'), /unknown sample format/);
  assert.throws(() => b.modulateSamples(payloads, 's16', 'planar'), /unknown layout/);
  assert.throws(() => b.modulateSamples(payloads, 's16', 'stream', longest, longest, s16.subarray(1)), /samples too short/);
  assert.throws(() => b.modulateSamples(payloads, 's16', 'sample', longest, S - 1), /samples too short/);
  assert.throws(() => b.modulateSamples(payloads.slice(1), 's16', 'stream'), /one payload per stream/);
  assert.throws(() => b.modulateSamples(payloads, 's16', 'stream', longest - 1), /needs \d+ samples/);   // FSKHIP_E_OVERFLOW
  b.close();
  sh.close();

  // modulateSamples -> demodulateSamples, the default configuration: every stream's frame comes back
  const frames = Array.from({ length: S }, (_, s) => letters(s));
  for (const fmt of ['s16', 'mulaw', 'alaw']) {
    for (const lay of ['stream', 'sample']) {
      const tx = new M.FSKBatch(S, {}), rx = new M.FSKBatch(S, {});
      const r = tx.modulateSamples(frames, fmt, lay);
      const got = rx.demodulateSamples(r.samples, fmt, lay, r.nPerStream, r.pitch);
      for (let s = 0; s < S; s++) assert.deepStrictEqual(Array.from(got.bytes[s]), Array.from(frames[s]), fmt + ' ' + lay + ': round trip ' + s);
      tx.close();
      rx.close();
    }
  }
  console.log('js egress gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'gpu') gpuTests().catch((e) => { console.error(e); process.exit(1); });
