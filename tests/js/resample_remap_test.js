'use strict';
// Upsampler / Downsampler of napi/filters.js through remap, snapshot and fromSnapshot (include/fskhip_next.h: fskhip_resampler_remap,
// _snapshot, _restore, _snapshot_info_get).
//   cpu: the surface, and the refusals that need no device.
//   gpu <up digest> <down digest>: an interpolator and a decimator -- 66 streams, factor 6, the default 97 taps -- filled by one
//        process call, then carried three ways with one map: remap(map), fromSnapshot(snapshot(), map) and fromSnapshot(snapshot(sel),
//        map2) with sel[map2] = map.  All three must give the sha256 the Python binding gives for remapped(map): over the state
//        behind the carry, the output of a further call and the state behind that (formulas shared with
//        tests/test_node_resample_remap.py, no random numbers).  The source is unchanged; a damaged image is refused.
// usage: node resample_remap_test.js cpu | gpu <up> <down>
const assert = require('assert');
const crypto = require('crypto');
const path = require('path');
const F = require(path.join(__dirname, '..', '..', 'napi', 'filters.js'));

const S = 66, L = 6;
const MAP = Array.from({ length: S + 5 }, (_, i) => (i % 9 === 4 ? -1 : (i * 29 + 3) % S));   // a permutation's start, clones, new streams
const SEL = Array.from({ length: S }, (_, r) => (r * 5 + 1) % S);                                // a permutation of the streams
const MAP2 = MAP.map((m) => (m < 0 ? -1 : SEL.indexOf(m)));

function bytesOf(a) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength); }
function mulawRows(m0, n, streams) {          // [streams][n]
  const a = new Uint8Array(n * streams);
  for (let s = 0; s < streams; s++) for (let m = 0; m < n; m++) a[s * n + m] = (s * 37 + (m0 + m) * 11 + ((m0 + m) * (m0 + m)) % 7) & 0xff;
  return a;
}
function floats(t0, n, streams) {             // [streams][n]
  const a = new Float32Array(streams * n);
  for (let s = 0; s < streams; s++) for (let t = 0; t < n; t++) a[s * n + t] = ((s * 131 + (t0 + t) * 29) % 2001 - 1000) / 1000;
  return a;
}

function cpuTests() {
  for (const C of [F.Upsampler, F.Downsampler]) {
    for (const m of ['remap', 'snapshot']) assert.strictEqual(typeof C.prototype[m], 'function', m);
    assert.strictEqual(typeof C.fromSnapshot, 'function');
    assert.throws(() => C.fromSnapshot(Buffer.alloc(8)), /fewer than a resampler snapshot header/);
    assert.throws(() => C.fromSnapshot(Buffer.alloc(64)), /not a resampler snapshot/);
  }
  assert.strictEqual(typeof F.resamplerSnapshotInfo, 'function');
  assert.throws(() => F.resamplerSnapshotInfo(Buffer.alloc(48)), /not a resampler snapshot/);
  console.log('js resample remap cpu tests ok');
}

function digestOf(h, step) {
  const d = crypto.createHash('sha256');
  d.update(bytesOf(h.state()));
  d.update(bytesOf(step(h)));
  d.update(bytesOf(h.state()));
  return d.digest('hex');
}

function carry(C, fill, step, want, direction) {
  const src = new C(L, S);
  fill(src);
  const before = src.state();
  const snap = src.snapshot(), part = src.snapshot(SEL);
  assert.ok(Buffer.isBuffer(snap) && snap.length % 16 === 0);
  const info = F.resamplerSnapshotInfo(snap);
  assert.deepStrictEqual([info.nStreams, info.direction, info.factor, info.nTaps, info.precision, info.history], [S, direction, L, 97, 0, src.history]);
  assert.deepStrictEqual(Array.from(info.taps), src.taps);
  const made = [src.remap(MAP), C.fromSnapshot(snap, MAP), C.fromSnapshot(part, MAP2)];
  for (const h of made) {
    assert.ok(h instanceof C && h.nStreams === MAP.length && h.history === src.history && h.factor === L);
    assert.deepStrictEqual(h.taps, src.taps);
    assert.strictEqual(digestOf(h, step), want, 'the Python binding computes something else');
    h.close();
  }
  const all = C.fromSnapshot(snap);             // no map: every record, in order
  assert.deepStrictEqual(all.state(), before);
  all.close();
  assert.deepStrictEqual(src.state(), before);  // the source is not changed
  const Other = C === F.Upsampler ? F.Downsampler : F.Upsampler;
  assert.throws(() => Other.fromSnapshot(snap), /the snapshot is of a resampler that goes/);
  assert.throws(() => src.remap([0, S]), /map\[1\] = 66, the source has 66 streams/);
  assert.throws(() => src.remap([]), /n_map is 0/);
  const bad = Buffer.from(snap);
  bad[bad.length - 40] ^= 4;
  assert.throws(() => C.fromSnapshot(bad), /checksum/);
  src.close();
}

function gpuTests(wantUp, wantDown) {
  carry(F.Upsampler, (h) => h.process(mulawRows(0, 60, S), 'mulaw'), (h) => h.process(mulawRows(60, 37, h.nStreams), 'mulaw'), wantUp, 0);
  carry(F.Downsampler, (h) => h.process(floats(0, 600, S), 's16'), (h) => h.process(floats(600, 37 * L, h.nStreams), 's16'), wantDown, 1);
  console.log('js resample remap gpu tests ok');
}

const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') gpuTests(process.argv[3], process.argv[4]); else cpuTests();
