'use strict';
// FSKBatch.remap through the N-API addon on the GPU (include/fskhip.h, fskhip_remap_streams): every continued stream of the
// remapped batch equals the control batch's stream map[i] after the cut -- bytes, per-call 'eod' counts, status -- and every
// new stream (-1) equals a freshly created batch fed the same samples.  usage: node remap_test.js gpu
const assert = require('assert');
const path = require('path');
const M = require(path.join(__dirname, '..', '..', 'napi', 'fsk-core.js'));

const S = 130;

function signals(nStreams, n, seed) {
  // two modulateData frames per stream behind a staggered lead-in
  const mod = new M.FSKBatch(nStreams, {});
  const pay = [];
  for (let s = 0; s < nStreams; s++) pay.push(Uint8Array.from([0x41 + (s % 26), (s * 7 + seed) & 0xff, seed & 0xff, 0x5a]));
  const frames = mod.modulateData(pay);
  mod.close();
  const x = new Float32Array(nStreams * n);
  for (let s = 0; s < nStreams; s++) {
    let at = (s * 37 + seed * 11) % 700;
    for (let k = 0; k < 2 && at + frames[s].length <= n; k++) {
      x.set(frames[s], s * n + at);
      at += frames[s].length + 200 + (s % 5) * 40;
    }
  }
  return x;
}

function rows(x, n, idx, a, b) {
  const out = new Float32Array(idx.length * (b - a));
  idx.forEach((r, i) => { if (r >= 0) out.set(x.subarray(r * n + a, r * n + b), i * (b - a)); });
  return out;
}

function gpuTests() {
  const N = 7200, cut = 3072;
  const x = signals(S, N, 3);
  const all = Array.from({ length: S }, (_, s) => s);
  const ctrl = new M.FSKBatch(S, {});
  const src = new M.FSKBatch(S, {});
  for (const [a, b] of [[0, 1000], [1000, cut]]) {
    ctrl.demodulateData(rows(x, N, all, a, b), b - a);
    src.demodulateData(rows(x, N, all, a, b), b - a);
  }
  const map = [];
  for (let i = 0; i < 97; i++) map.push(i % 11 === 5 ? -1 : (i * 53 + 17) % S);   // permutes, drops, duplicates; new slots
  const dst = src.remap(map);
  const fidx = map.map((v, i) => (v < 0 ? i : -1)).filter((i) => i >= 0);
  const fresh = new M.FSKBatch(fidx.length, {});
  const y = signals(fidx.length, N - cut, 9);
  const fall = Array.from({ length: fidx.length }, (_, j) => j);
  let off = cut, yoff = 0;
  for (const c of [1500, N - cut - 1500]) {
    const cr = ctrl.demodulateData(rows(x, N, all, off, off + c), c);
    const din = rows(x, N, map, off, off + c);
    fidx.forEach((i, j) => din.set(y.subarray(j * (N - cut) + yoff, j * (N - cut) + yoff + c), i * c));
    const dr = dst.demodulateData(din, c);
    const fr = fresh.demodulateData(rows(y, N - cut, fall, yoff, yoff + c), c);
    map.forEach((s, i) => {
      if (s < 0) return;
      assert.deepStrictEqual(Array.from(dr.bytes[i]), Array.from(cr.bytes[s]), 'bytes ' + i);
      assert.strictEqual(dr.eod[i], cr.eod[s], 'eod ' + i);
      assert.deepStrictEqual(dst.getStatus(i), ctrl.getStatus(s), 'status ' + i);
    });
    fidx.forEach((i, j) => {
      assert.deepStrictEqual(Array.from(dr.bytes[i]), Array.from(fr.bytes[j]), 'new stream bytes ' + i);
      assert.strictEqual(dr.eod[i], fr.eod[j]);
      // (fp32, one shared configuration: a new stream joins the batch's free-running I/Q frame, as at reset -- its two status
      // reals agree to fp32 rounding, include/fskhip.h)
      const a = dst.getStatus(i), b = fresh.getStatus(j);
      for (const k of ['silenceThreshold', 'agcGain']) {
        assert.ok(Math.abs(a[k] - b[k]) <= 1e-5 * Math.abs(b[k]), k + ' ' + a[k] + ' ' + b[k]);
        delete a[k]; delete b[k];
      }
      assert.deepStrictEqual(a, b, 'new stream status ' + i);
    });
    off += c; yoff += c;
  }
  let decoded = 0;
  for (let i = 0; i < 97; i++) decoded += dst.getStatus(i).syncDetections;
  assert.ok(decoded > 0);
  assert.throws(() => src.remap([S]), /source has 130 streams/);
  [ctrl, src, dst, fresh].forEach((b) => b.close());
  console.log('js remap gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'gpu') gpuTests();
