'use strict';
// CaptureConverter / PlaybackConverter of napi/filters.js through remap, snapshot and fromSnapshot (include/fskhip_next.h:
// fskhip_ratecvt_remap, _snapshot, _restore, _snapshot_info_get).
//   cpu: the surface, and the refusals that need no device.
//   gpu: a capture converter 44.1 -> 48 kHz and a playback converter 48 -> 44.1 kHz, at 5 and at 65 streams, filled by one
//        processAny of 131 samples (so the handle stands between two period boundaries), then carried three ways with one map:
//        remap(map), fromSnapshot(snapshot(), map) and fromSnapshot(snapshot(sel), map2) with sel[map2] = map.  Each must equal the
//        by-hand carry -- a new object, setState of the rows taken through the map, setPosition -- byte for byte: the state behind
//        the carry, the position, and output, state and position over two further processAny calls of 1 and 129 samples.  The
//        source is unchanged; a damaged image, an image of the other direction and a bad map are refused.  No random numbers.
// usage: node ratecvt_remap_test.js cpu | gpu
const assert = require('assert');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

function bytesOf(a) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength); }
function s16Rows(m0, n, streams) {            // [streams][n]
  const a = new Int16Array(n * streams);
  for (let s = 0; s < streams; s++) for (let m = 0; m < n; m++) a[s * n + m] = ((s * 3701 + (m0 + m) * 1117 + ((m0 + m) * (m0 + m)) % 71) % 60001) - 30000;
  return a;
}
function floats(t0, n, streams) {             // [streams][n]
  const a = new Float32Array(streams * n);
  for (let s = 0; s < streams; s++) for (let t = 0; t < n; t++) a[s * n + t] = ((s * 131 + (t0 + t) * 29) % 2001 - 1000) / 1000;
  return a;
}

function cpuTests() {
  for (const C of [F.CaptureConverter, F.PlaybackConverter]) {
    for (const m of ['remap', 'snapshot', 'state', 'setState', 'setPosition']) assert.strictEqual(typeof C.prototype[m], 'function', m);
    assert.strictEqual(typeof C.fromSnapshot, 'function');
    assert.throws(() => C.fromSnapshot(Buffer.alloc(8)), /fewer than a rate converter snapshot header/);
    assert.throws(() => C.fromSnapshot(Buffer.alloc(64)), /not a rate converter snapshot/);
  }
  assert.strictEqual(typeof F.ratecvtSnapshotInfo, 'function');
  assert.throws(() => F.ratecvtSnapshotInfo(Buffer.alloc(64)), /not a rate converter snapshot/);
  assert.throws(() => F.ratecvtSnapshotInfo(Buffer.alloc(63)), /fewer than a rate converter snapshot header/);
  const resampler = Buffer.alloc(64);           // a resampler's magic names itself
  resampler.writeUInt32LE(0x524B5346, 0);
  assert.throws(() => F.ratecvtSnapshotInfo(resampler), /is a resampler snapshot's/);
  console.log('js ratecvt remap cpu tests ok');
}

function rowsThrough(state, H, map) {           // the by-hand carry's rows: row i = row map[i] of state, zeros for -1
  const out = new Float32Array(map.length * H);
  map.forEach((m, i) => { if (m >= 0) out.set(state.subarray(m * H, (m + 1) * H), i * H); });
  return out;
}

function carry(C, rates, S, fill, step, direction) {
  const MAP = Array.from({ length: S + 3 }, (_, i) => (i % 4 === 2 ? -1 : (i * 29 + 3) % S));   // a permutation's start, clones, new streams
  const SEL = Array.from({ length: S }, (_, r) => (r * 3 + 1) % S);                                // a permutation of the streams (S is no multiple of 3)
  const MAP2 = MAP.map((m) => (m < 0 ? -1 : SEL.indexOf(m)));
  const src = new C(rates[0], rates[1], S);
  fill(src);
  const before = src.state(), pos = src.position;
  assert.ok(pos !== 0 && pos === 131 % src.down);
  const snap = src.snapshot(), part = src.snapshot(SEL);
  assert.ok(Buffer.isBuffer(snap) && snap.length % 16 === 0 && snap.length === Math.ceil((64 + 8 * 2561 + 4 * S * src.history) / 16) * 16);
  const info = F.ratecvtSnapshotInfo(snap);
  assert.deepStrictEqual([info.nStreams, info.direction, info.up, info.down, info.nTaps, info.precision, info.history, info.position],
    [S, direction, src.up, src.down, 2561, 0, src.history, pos]);
  assert.deepStrictEqual(Array.from(info.taps), src.taps);
  const made = [src.remap(MAP), C.fromSnapshot(snap, MAP, { device: 0, inRate: rates[0], outRate: rates[1] }), C.fromSnapshot(part, MAP2, 0)];
  made.forEach((h, k) => {
    const hand = new C(rates[0], rates[1], MAP.length);
    hand.setState(rowsThrough(before, src.history, MAP));
    hand.setPosition(pos);
    assert.ok(h instanceof C && h.nStreams === MAP.length && h.history === src.history && h.up === src.up && h.down === src.down);
    assert.deepStrictEqual([h.inRate, h.outRate], k < 2 ? rates : [src.down, src.up]);   // an image knows up and down, not the rates
    assert.deepStrictEqual(h.taps, src.taps);
    assert.strictEqual(h.position, pos);
    assert.ok(bytesOf(h.state()).equals(bytesOf(hand.state())), 'state behind the carry, way ' + k);
    let t0 = 131;
    for (const n of [1, 129]) {
      assert.ok(bytesOf(step(h, t0, n)).equals(bytesOf(step(hand, t0, n))), 'output of ' + n + ', way ' + k);
      assert.ok(bytesOf(h.state()).equals(bytesOf(hand.state())) && h.position === hand.position, 'state after ' + n + ', way ' + k);
      t0 += n;
    }
    h.close(); hand.close();
  });
  const all = C.fromSnapshot(snap);             // no map: every record, in order
  assert.deepStrictEqual(all.state(), before);
  assert.strictEqual(all.position, pos);
  all.close();
  const viaBase = Object.getPrototypeOf(C).fromSnapshot(snap);   // the class the two share picks from the image
  assert.ok(viaBase instanceof C && viaBase.nStreams === S);
  viaBase.close();
  assert.deepStrictEqual(src.state(), before);  // the source is not changed
  assert.strictEqual(src.position, pos);
  const Other = C === F.CaptureConverter ? F.PlaybackConverter : F.CaptureConverter;
  assert.throws(() => Other.fromSnapshot(snap), /the snapshot is of a rate converter for/);
  assert.throws(() => C.fromSnapshot(snap, null, { inRate: 8000, outRate: 48000 }), /the snapshot converts by/);
  assert.throws(() => src.remap([0, S]), new RegExp('map\\[1\\] = ' + S + ', the source has ' + S + ' streams'));
  assert.throws(() => src.remap([-2]), /map\[0\] = -2/);
  assert.throws(() => src.remap([]), /n_map is 0/);
  assert.throws(() => src.snapshot([S]), /sel\[0\] = /);
  assert.throws(() => C.fromSnapshot(snap, [0, S]), new RegExp('map\\[1\\] = ' + S + ', the snapshot has ' + S + ' records'));
  assert.throws(() => C.fromSnapshot(snap, []), /n_map is 0/);
  const bad = Buffer.from(snap);
  bad[bad.length - 40] ^= 4;
  assert.throws(() => C.fromSnapshot(bad), /checksum/);
  assert.throws(() => F.ratecvtSnapshotInfo(snap.subarray(0, snap.length - 16)), /do not match the layout/);
  src.close();
}

function gpuTests() {
  for (const S of [5, 65]) {
    carry(F.CaptureConverter, [44100, 48000], S, (h) => h.processAny(s16Rows(0, 131, S), 's16'), (h, t0, n) => h.processAny(s16Rows(t0, n, h.nStreams), 's16'), 0);
    carry(F.PlaybackConverter, [48000, 44100], S, (h) => h.processAny(floats(0, 131, S), 's16'), (h, t0, n) => h.processAny(floats(t0, n, h.nStreams), 's16'), 1);
  }
  console.log('js ratecvt remap gpu tests ok');
}

const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') gpuTests(); else cpuTests();
