'use strict';
// Stream snapshots through the N-API addon on the GPU (include/fskhip.h, fskhip_snapshot_streams / fskhip_restore_streams):
// FSKBatch.snapshot() -> Buffer -> FSKBatch.fromSnapshot round trip with the source destroyed in between, and
// FSKBatchSharded.remap on devices [0, 0] -> [0, 0, 0], against an uninterrupted FSKBatch: bytes, per-call 'eod' counts, status.
// usage: node snapshot_test.js gpu
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

// feed ctrl its rows and dst the rows its map names; every continued stream equals the control's
async function follow(ctrl, dst, map, x, N, cut, statusOf) {
  const all = Array.from({ length: S }, (_, s) => s);
  let off = cut, decoded = 0;
  for (const c of [1500, N - cut - 1500]) {
    const cr = ctrl.demodulateData(rows(x, N, all, off, off + c), c);
    const dr = await dst.demodulateData(rows(x, N, map, off, off + c), c);
    map.forEach((s, i) => {
      if (s < 0) return;
      assert.deepStrictEqual(Array.from(dr.bytes[i]), Array.from(cr.bytes[s]), 'bytes ' + i);
      assert.strictEqual(dr.eod[i], cr.eod[s], 'eod ' + i);
      assert.deepStrictEqual(statusOf(i), ctrl.getStatus(s), 'status ' + i);
      decoded += dr.bytes[i].length;
    });
    off += c;
  }
  assert.ok(decoded > 0);
}

async function gpuTests() {
  const N = 7200, cut = 3072;
  const x = signals(S, N, 3);
  const all = Array.from({ length: S }, (_, s) => s);
  const upToCut = (b) => { for (const [a, e] of [[0, 1000], [1000, cut]]) b.demodulateData(rows(x, N, all, a, e), e - a); return b; };

  // FSKBatch: snapshot, destroy, restore from the bytes alone
  let ctrl = upToCut(new M.FSKBatch(S, {}));
  const src = upToCut(new M.FSKBatch(S, {}));
  const buf = src.snapshot();
  assert.ok(Buffer.isBuffer(buf));
  assert.ok(buf.equals(src.snapshot()), 'two snapshots of the same state are byte-identical');
  src.close();
  const info = M.snapshotInfo(buf);
  assert.strictEqual(info.nStreams, S);
  assert.strictEqual(info.precision, M.PRECISION_F32);
  assert.strictEqual(info.demodulationCalls, 2);
  assert.strictEqual(info.totalSamplesProcessed, cut);
  assert.strictEqual(buf.length, 352 + S * info.recordBytes);
  const map = [];
  for (let i = 0; i < 97; i++) map.push(i % 11 === 5 ? -1 : (i * 53 + 17) % S);   // permutes, drops, duplicates; new slots
  const whole = M.FSKBatch.fromSnapshot(Buffer.from(buf));      // (a copy: nothing but the bytes)
  assert.strictEqual(whole.nStreams, S);
  all.forEach((s) => assert.deepStrictEqual(whole.getStatus(s), ctrl.getStatus(s)));
  whole.close();
  const dst = M.FSKBatch.fromSnapshot(buf, map);
  await follow(ctrl, dst, map, x, N, cut, (i) => dst.getStatus(i));
  assert.throws(() => M.FSKBatch.fromSnapshot(buf, [S]), /snapshot has 130 records/);
  const damaged = Buffer.from(buf);
  damaged[1000] ^= 1;
  assert.throws(() => M.FSKBatch.fromSnapshot(damaged), /checksum/);
  dst.close();
  ctrl.close();

  // FSKBatchSharded on [0, 0]: remap across shards onto [0, 0, 0]
  ctrl = upToCut(new M.FSKBatch(S, {}));
  const sh = new M.FSKBatchSharded(S, {}, { devices: [0, 0] });
  for (const [a, e] of [[0, 1000], [1000, cut]]) await sh.demodulateData(rows(x, N, all, a, e), e - a);
  const whole2 = sh.snapshot();
  assert.strictEqual(M.snapshotInfo(whole2).nStreams, S);
  const next = sh.remap(map, undefined, { devices: [0, 0, 0] });
  assert.strictEqual(next.shards.length, 3);
  assert.strictEqual(next.nStreams, map.length);
  sh.close();
  await follow(ctrl, next, map, x, N, cut, (i) => next.getStatus(i));
  next.close();
  ctrl.close();
  console.log('js snapshot gpu tests ok');
}

if ((process.argv[2] || 'gpu') === 'gpu') gpuTests().catch((e) => { console.error(e); process.exit(1); });
